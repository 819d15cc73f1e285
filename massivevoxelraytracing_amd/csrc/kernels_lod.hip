// kernels_lod.hip -- level of detail per ray inside one octree (mvrt_svo_lod_prepare, mvrt_trace_batch_cone, mvrt_render_primary_lod).
// The kernels are the cone walk of include/mvrt/device.hpp (DeviceOctree::intersectConeEx), one ray per lane, the stack in LDS, launched as kTraceRange is
// (kernels_range.hip); the colour of a stopped ray comes from the attribute pyramid through DeviceLod::lookup.  The pyramid is the coarse listing of
// kernels_coarsen.hip run once per level on the sorted voxel list: every level's sums are taken over the voxels themselves, never over the level below.  The
// streaming kernels (traverse_stream.h) are not involved.
#include <string.h>

#include "../../include/mvrt/device.hpp"
#include "launch.h"

#define LOD_WAVE 64

// ---- the pyramid --------------------------------------------------------------------------------------------------------------------------------------
int lodBuild( const uint64_t* morton, const uint2* attrs, uint32_t n, uint32_t levels, LodPyramid* out, hipStream_t stream )
{
	LodPyramid p;
	for( uint32_t L = 1; L < levels; L++ )
		if( coarseCells( morton, attrs, n, (int)( levels - L ), p.codes[L], p.attrs[L], p.counts[L], &p.n[L], stream ) ) return 1; // (p releases what it holds)
	p.ready = 1;
	*out = std::move( p );
	return 0;
}

// ---- mvrt_trace_batch_cone ----------------------------------------------------------------------------------------------------------------------------
struct ConeIO
{
	const float *rox, *roy, *roz, *rdx, *rdy, *rdz;
	const float *coneA, *coneB;
	float* t;
	int32_t* nMajor;
	uint32_t* level;
	uint64_t* cellCode;
	uint32_t* index;
	uint2* attrib;
	uint32_t* descents;
};
// hasLod == 0: lod is not read (io.index and io.attrib are null)
__global__ void __launch_bounds__( LOD_WAVE ) kTraceCone( mvrt_device_octree view, mvrt_device_lod lodView, uint32_t hasLod, uint64_t n, ConeIO io )
{
	extern __shared__ mvrt::StackEntry coneStack[]; // [lane][level]
	const uint64_t i = (uint64_t)blockIdx.x * LOD_WAVE + threadIdx.x;
	if( i >= n ) return;
	const mvrt::DeviceOctree oct( view );
	const float3 ro = make_float3( io.rox[i], io.roy[i], io.roz[i] );
	const float3 rd = make_float3( io.rdx[i], io.rdy[i], io.rdz[i] );
	float t;
	int nm;
	uint32_t lv, de;
	uint64_t code;
	oct.intersectConeEx( coneStack + threadIdx.x * view.levels, ro, rd, io.coneA[i], io.coneB[i], &t, &nm, &lv, &code, &de );
	io.t[i] = t;
	if( io.nMajor ) io.nMajor[i] = nm;
	if( io.level ) io.level[i] = lv;
	if( io.cellCode ) io.cellCode[i] = code;
	if( io.descents ) io.descents[i] = de;
	if( hasLod && ( io.index || io.attrib ) )
	{
		const mvrt::DeviceLod lod( lodView );
		uint32_t idx = 0;
		uint2 a = make_uint2( 0u, 0u );
		if( lv != 0u ) // a hit
		{
			if( lod.lookup( lv, code, &idx ) ) a = lod.attrib( lv, idx );
			else idx = 0xFFFFFFFFu; // (a cell the octree has and the pyramid lacks: they do not describe the same voxels)
		}
		if( io.index ) io.index[i] = idx;
		if( io.attrib ) io.attrib[i] = a;
	}
}
static int coneBlocks( const char* who, uint64_t n, uint64_t* blocks )
{
	*blocks = ( n + LOD_WAVE - 1 ) / LOD_WAVE;
	if( *blocks > 0x7FFFFFFFull )
	{
		mvrtSetError( "%s: %llu rays exceed one launch (2^37 - 64)", who, (unsigned long long)n );
		return 1;
	}
	return 0;
}
int launchTraceCone( const mvrt_device_octree& view, const mvrt_device_lod* lod, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy,
					 const float* rdz, const float* coneA, const float* coneB, float* t, int32_t* nMajor, uint32_t* level, uint64_t* cellCode, uint32_t* index, uint32_t* attrib,
					 uint32_t* descents, hipStream_t stream )
{
	if( n == 0 ) return 0;
	uint64_t blocks;
	if( coneBlocks( "mvrt_trace_batch_cone", n, &blocks ) ) return 1;
	mvrt_device_lod lv;
	memset( &lv, 0, sizeof( lv ) );
	if( lod ) lv = *lod;
	const ConeIO io = { rox, roy, roz, rdx, rdy, rdz, coneA, coneB, t, nMajor, level, cellCode, lod ? index : nullptr, lod ? (uint2*)attrib : nullptr, descents };
	hipLaunchKernelGGL( kTraceCone, dim3( (uint32_t)blocks ), dim3( LOD_WAVE ), LOD_WAVE * view.levels * sizeof( mvrt::StackEntry ), stream, view, lv, lod ? 1u : 0u, n, io );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// ---- mvrt_render_primary_lod --------------------------------------------------------------------------------------------------------------------------
struct RenderLodIO
{
	mvrt::CameraPinhole cam;
	int W, H;
	float coneB;
	uchar4* rgba;
	float* t;
	int32_t* nMajor;
	uint32_t* level;
	uint32_t* descents;
};
// One pixel per lane, row-major: the ray of mvrt_render_primary (the reference's `render`, voxKernel.cu:437-483) with the cone { 0, coneB }
__global__ void __launch_bounds__( LOD_WAVE ) kRenderLod( mvrt_device_octree view, mvrt_device_lod lodView, uint32_t hasLod, RenderLodIO io )
{
	MVRT_DEVICE_FP_STRICT
	extern __shared__ mvrt::StackEntry lodStack[]; // [lane][level]
	const uint64_t i = (uint64_t)blockIdx.x * LOD_WAVE + threadIdx.x;
	if( i >= (uint64_t)io.W * (uint64_t)io.H ) return;
	const mvrt::DeviceOctree oct( view );
	float3 ro, rd;
	io.cam.shoot( &ro, &rd, (int)( i % (uint64_t)io.W ), (int)( i / (uint64_t)io.W ), 0.5f, 0.5f, io.W, io.H ); // voxKernel.cu:455
	float t;
	int nm;
	uint32_t lv, de;
	uint64_t code;
	oct.intersectConeEx( lodStack + threadIdx.x * view.levels, ro, rd, 0.0f, io.coneB, &t, &nm, &lv, &code, &de );
	if( io.rgba )
	{
		uchar4 c = make_uchar4( 0, 0, 0, 255 );
		if( t != mvrt::detail::kMaxFloat ) // voxKernel.cu:462-478
		{
			if( hasLod )
			{
				const mvrt::DeviceLod lod( lodView );
				uint32_t idx;
				if( lod.lookup( lv, code, &idx ) ) c = lod.color( lv, idx );
			}
			else
			{
				const float3 hn = mvrt::getHitN( nm, rd );
				c = make_uchar4( (uint8_t)( 255 * ( ( hn.x + 1.0f ) * 0.5f ) + 0.5f ), (uint8_t)( 255 * ( ( hn.y + 1.0f ) * 0.5f ) + 0.5f ),
								 (uint8_t)( 255 * ( ( hn.z + 1.0f ) * 0.5f ) + 0.5f ), 255 );
			}
		}
		io.rgba[i] = c;
	}
	if( io.t ) io.t[i] = t;
	if( io.nMajor ) io.nMajor[i] = nm;
	if( io.level ) io.level[i] = lv;
	if( io.descents ) io.descents[i] = de;
}
int launchRenderLod( const mvrt_device_octree& view, const mvrt_device_lod* lod, const float camera[15], int W, int H, float coneB, uchar4* rgba, float* t, int32_t* nMajor,
					 uint32_t* level, uint32_t* descents, hipStream_t stream )
{
	const uint64_t n = (uint64_t)W * (uint64_t)H;
	if( n == 0 ) return 0;
	uint64_t blocks;
	if( coneBlocks( "mvrt_render_primary_lod", n, &blocks ) ) return 1;
	mvrt_device_lod lv;
	memset( &lv, 0, sizeof( lv ) );
	if( lod ) lv = *lod;
	RenderLodIO io;
	io.cam = mvrt::CameraPinhole( camera );
	io.W = W;
	io.H = H;
	io.coneB = coneB;
	io.rgba = rgba;
	io.t = t;
	io.nMajor = nMajor;
	io.level = level;
	io.descents = descents;
	hipLaunchKernelGGL( kRenderLod, dim3( (uint32_t)blocks ), dim3( LOD_WAVE ), LOD_WAVE * view.levels * sizeof( mvrt::StackEntry ), stream, view, lv, lod ? 1u : 0u, io );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
