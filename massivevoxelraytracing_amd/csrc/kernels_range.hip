// kernels_range.hip -- distance-limited rays (mvrt_trace_batch_range) and the per-face ambient occlusion bake (mvrt_svo_surface_ao).
// Both kernels are the per-lane walk of include/mvrt/device.hpp (DeviceOctree::walk<true>), one ray per lane, the stack in LDS: view.levels entries of
// 16 bytes per lane, so a wave of a 256^3 octree holds 8 KiB and one of a 2048^3 octree 11 KiB.  The streaming kernels
// (traverse_stream.h) are not involved.
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/mvrt/device.hpp"
#include "launch.h"

#define RANGE_WAVE 64

// ---- mvrt_trace_batch_range ------------------------------------------------------------------------------------------------------------------------
struct RangeIO
{
	const float *rox, *roy, *roz, *rdx, *rdy, *rdz;
	const uint8_t* isShadow;
	const float* tMax;
	float* t;
	int32_t* nMajor;
	uint32_t* vIndex;
	uint32_t* descents;
};
__global__ void __launch_bounds__( RANGE_WAVE ) kTraceRange( mvrt_device_octree view, uint64_t n, RangeIO io )
{
	extern __shared__ mvrt::StackEntry rangeStack[]; // [lane][level]
	const uint64_t i = (uint64_t)blockIdx.x * RANGE_WAVE + threadIdx.x;
	if( i >= n ) return;
	const mvrt::DeviceOctree oct( view );
	const float3 ro = make_float3( io.rox[i], io.roy[i], io.roz[i] );
	const float3 rd = make_float3( io.rdx[i], io.rdy[i], io.rdz[i] );
	const bool sh = io.isShadow ? io.isShadow[i] != 0 : false;
	float t;
	int nm;
	uint32_t vi, de;
	oct.intersectRangeEx( rangeStack + threadIdx.x * view.levels, ro, rd, io.tMax[i], &t, &nm, &vi, sh, &de );
	io.t[i] = t;
	if( io.nMajor ) io.nMajor[i] = nm;
	if( io.vIndex ) io.vIndex[i] = vi;
	if( io.descents ) io.descents[i] = de;
}
int launchTraceRange( const mvrt_device_octree& view, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz,
					  const uint8_t* isShadow, const float* tMax, float* t, int32_t* nMajor, uint32_t* vIndex, uint32_t* descents, hipStream_t stream )
{
	if( n == 0 ) return 0;
	const uint64_t blocks = ( n + RANGE_WAVE - 1 ) / RANGE_WAVE;
	if( blocks > 0x7FFFFFFFull )
	{
		mvrtSetError( "mvrt_trace_batch_range: %llu rays exceed one launch (2^37 - 64)", (unsigned long long)n );
		return 1;
	}
	const RangeIO io = { rox, roy, roz, rdx, rdy, rdz, isShadow, tMax, t, nMajor, vIndex, descents };
	hipLaunchKernelGGL( kTraceRange, dim3( (uint32_t)blocks ), dim3( RANGE_WAVE ), RANGE_WAVE * view.levels * sizeof( mvrt::StackEntry ), stream, view, n, io );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// ---- ambient occlusion ------------------------------------------------------------------------------------------------------------------------------
// sampleLambertian + GetOrthonormalBasis (renderCommon.hpp:119-151) in the deterministic math, the operations of kernels_rt.hip's in their order; this
// translation unit is compiled without contraction on the host side too, so the host table has the bits the path tracer's kernel would give
static f3 aoSampleLambertian( float a, float b, f3 Ng )
{
	float r = sqrtf( a );
	float theta = b * MVRT_PI * 2.0f;
	float sn, cs;
	mvrt_sincos( theta, &sn, &cs );
	float x = r * cs;
	float y = r * sn;
	float z = sqrtf( smax( 1.0f - a, 0.0f ) );
	const float sign = copysignf( 1.0f, Ng.z );
	const float aa = -1.0f / ( sign + Ng.z );
	const float bb = Ng.x * Ng.y * aa;
	f3 xaxis = mk3( 1.0f + sign * Ng.x * Ng.x * aa, sign * bb, -sign * Ng.x );
	f3 yaxis = mk3( bb, sign + Ng.y * Ng.y * aa, -Ng.y );
	return xaxis * x + yaxis * y + Ng * z;
}
// directions in the order of mvrt.h: 0 -Y, 1 +Y, 2 -Z, 3 +X, 4 +Z, 5 -X
static const int kAoAxis[6] = { 1, 1, 2, 0, 2, 0 };
static const int kAoPositive[6] = { 0, 1, 0, 1, 1, 0 };
bool aoSamplesOk( int samples ) { return samples >= 1 && samples <= 256 && ( samples & ( samples - 1 ) ) == 0; }
void aoDirections( int samples, float* dirs )
{
	for( int d = 0; d < 6; d++ )
	{
		float n[3] = { 0.0f, 0.0f, 0.0f };
		n[kAoAxis[d]] = kAoPositive[d] ? 1.0f : -1.0f;
		for( int k = 0; k < samples; k++ )
		{
			const float a = ( (float)k + 0.5f ) / (float)samples;				  // exact: K is a power of two
			const float b = (float)( reverseBits32( (uint32_t)k ) >> 8 ) / 16777216.0f; // the base-2 radical inverse of k < 256, exact
			const f3 v = aoSampleLambertian( a, b, mk3( n[0], n[1], n[2] ) );
			float* o = dirs + ( (size_t)d * samples + k ) * 3;
			o[0] = v.x;
			o[1] = v.y;
			o[2] = v.z;
		}
	}
}

// the lowest entry with faceVoxel >= nVoxels or faceDir >= 6 (~0 = none)
__global__ void __launch_bounds__( 256 ) kAoValidate( uint64_t nFaces, const uint32_t* __restrict__ faceVoxel, const uint8_t* __restrict__ faceDir, uint32_t nVoxels,
													   unsigned long long* __restrict__ lowestBad )
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if( i >= nFaces ) return;
	if( faceVoxel[i] >= nVoxels || faceDir[i] >= 6 ) atomicMin( lowestBad, (unsigned long long)i );
}

// One wave per block.  K < 64: the wave bakes 64 / K consecutive faces, lane = face * K + sample; K >= 64: one face, K / 64 rounds of 64 samples.  The
// entries were validated (kAoValidate) before this kernel is launched.
__global__ void __launch_bounds__( RANGE_WAVE ) kSurfaceAo( mvrt_device_octree view, const uint64_t* __restrict__ morton, uint64_t nFaces, const uint32_t* __restrict__ faceVoxel,
															 const uint8_t* __restrict__ faceDir, uint32_t samples, uint32_t log2Samples, float radius,
															 const float* __restrict__ dirs, uint16_t* __restrict__ open )
{
	MVRT_DEVICE_FP_STRICT
	extern __shared__ mvrt::StackEntry aoStack[]; // [lane][level]
	const mvrt::DeviceOctree oct( view );
	const uint32_t lane = threadIdx.x;
	const uint32_t facesPerWave = samples < RANGE_WAVE ? RANGE_WAVE >> log2Samples : 1u;
	const uint32_t rounds = samples < RANGE_WAVE ? 1u : samples >> 6;
	const uint32_t sub = samples < RANGE_WAVE ? lane >> log2Samples : 0u; // the lane's face within the wave
	const uint64_t face = (uint64_t)blockIdx.x * facesPerWave + sub;
	const bool valid = face < nFaces;
	float3 ro = make_float3( 0.0f, 0.0f, 0.0f );
	uint32_t d = 0;
	if( valid )
	{
		d = faceDir[face];
		const uint64_t code = morton[faceVoxel[face]];
		uint32_t c2[3] = { 2u * compactBy3( code ) + 1u, 2u * compactBy3( code >> 1 ) + 1u, 2u * compactBy3( code >> 2 ) + 1u };
		// the face centre in half voxels: the in-plane axes at the voxel's middle, the normal axis on the face
		const uint32_t axis = ( d < 2u ) ? 1u : ( ( d == 2u || d == 4u ) ? 2u : 0u );
		const bool positive = d == 1u || d == 3u || d == 4u;
		if( axis == 0u ) c2[0] += positive ? 1u : ~0u;
		else if( axis == 1u ) c2[1] += positive ? 1u : ~0u;
		else c2[2] += positive ? 1u : ~0u;
		const float h = 0.5f * view.dps;
		ro = make_float3( view.lower[0] + (float)c2[0] * h, view.lower[1] + (float)c2[1] * h, view.lower[2] + (float)c2[2] * h );
	}
	uint32_t count = 0;
	for( uint32_t r = 0; r < rounds; r++ )
	{
		bool isOpen = false;
		if( valid )
		{
			const uint32_t k = samples < RANGE_WAVE ? ( lane & ( samples - 1u ) ) : r * RANGE_WAVE + lane;
			const float* v = dirs + ( (size_t)d * samples + k ) * 3;
			isOpen = !oct.occluded( aoStack + lane * view.levels, ro, make_float3( v[0], v[1], v[2] ), radius );
		}
		const unsigned long long b = __ballot( isOpen );
		if( samples < RANGE_WAVE ) count = (uint32_t)__popcll( ( b >> ( sub << log2Samples ) ) & ( ( 1ull << samples ) - 1ull ) );
		else count += (uint32_t)__popcll( b );
	}
	if( valid && ( lane & ( ( samples < RANGE_WAVE ? samples : RANGE_WAVE ) - 1u ) ) == 0u ) open[face] = (uint16_t)count;
}

// blocks: the lowest bad entry goes back to the host before anything is written, and the scratch (that word and the direction table) is released on return
int surfaceAo( const mvrt_device_octree& view, const uint64_t* morton, uint64_t nFaces, const uint32_t* faceVoxel, const uint8_t* faceDir, int samples, float radius,
			   uint16_t* open, hipStream_t stream )
{
	if( nFaces == 0 ) return 0;
	const uint64_t tableBytes = (uint64_t)6 * samples * 3 * sizeof( float );
	std::vector<float> table( (size_t)6 * samples * 3 );
	aoDirections( samples, table.data() );
	DevBuf scratch; // { lowest bad entry (8 bytes, padded to 16), directions }
	if( scratch.alloc( 16 + tableBytes ) ) return 1;
	unsigned long long* lowestBad = scratch.as<unsigned long long>();
	float* dirs = (float*)( (uint8_t*)scratch.p + 16 );
	MVRT_HIP( hipMemsetAsync( lowestBad, 0xFF, 16, stream ) );
	MVRT_HIP( hipMemcpyAsync( dirs, table.data(), tableBytes, hipMemcpyHostToDevice, stream ) );
	const uint64_t vBlocks = ( nFaces + 255 ) / 256;
	const uint32_t facesPerWave = samples < RANGE_WAVE ? RANGE_WAVE / samples : 1;
	const uint64_t blocks = ( nFaces + facesPerWave - 1 ) / facesPerWave;
	if( vBlocks > 0x7FFFFFFFull || blocks > 0x7FFFFFFFull )
	{
		mvrtSetError( "mvrt_svo_surface_ao: %llu faces exceed one launch", (unsigned long long)nFaces );
		return 1;
	}
	hipLaunchKernelGGL( kAoValidate, dim3( (uint32_t)vBlocks ), dim3( 256 ), 0, stream, nFaces, faceVoxel, faceDir, view.numberOfVoxels, lowestBad );
	MVRT_HIP( hipGetLastError() );
	unsigned long long bad = 0;
	MVRT_HIP( hipMemcpyAsync( &bad, lowestBad, sizeof( bad ), hipMemcpyDeviceToHost, stream ) );
	MVRT_HIP( hipStreamSynchronize( stream ) );
	if( bad != ~0ull )
	{
		uint32_t v = 0;
		uint8_t d = 0;
		MVRT_HIP( hipMemcpy( &v, faceVoxel + bad, sizeof( v ), hipMemcpyDeviceToHost ) ); // (default stream, both: the caller's arrays, behind the hipStreamSynchronize( stream ) above)
		MVRT_HIP( hipMemcpy( &d, faceDir + bad, sizeof( d ), hipMemcpyDeviceToHost ) );
		mvrtSetError( "mvrt_svo_surface_ao: entry %llu is out of range (faceVoxel %u of %u voxels, faceDir %u of 6); nothing was written", bad, v, view.numberOfVoxels,
					  (unsigned)d );
		return 1;
	}
	uint32_t log2Samples = 0;
	while( ( 1 << log2Samples ) < samples ) log2Samples++;
	hipLaunchKernelGGL( kSurfaceAo, dim3( (uint32_t)blocks ), dim3( RANGE_WAVE ), RANGE_WAVE * view.levels * sizeof( mvrt::StackEntry ), stream, view, morton, nFaces, faceVoxel,
						faceDir, (uint32_t)samples, log2Samples, radius, dirs, open );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( stream ) ); // (the table is released on return)
	return 0;
}
