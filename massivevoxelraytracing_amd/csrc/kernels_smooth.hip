// kernels_smooth.hip -- constrained surface nets on the welded voxel mesh (mvrt_svo_surface_smooth, mvrt.h): the faces, vertices and indices of
// mvrt_svo_surface_mesh, every vertex relaxed towards the mean of its edge neighbours inside a box around its lattice corner.  All of it in integers (steps of
// 1 / 256 cell), a Jacobi iteration over two buffers, so the result does not depend on the schedule; the one conversion to float is smoothPosition.
//
//   weld        the host steps of kernels_surface.hip (surface_weld.h): masks, face offsets, corner keys, the SurfaceWeld record, faceDir and indices.
//   neighbours  kSmoothNeighbours, one thread per sorted corner; the head of a run of equal keys owns the vertex and walks its run (the corners of the faces
//               that meet there, 24 at the most).  A corner k of face f has the neighbours indices[4 f + ( ( k +- 1 ) & 3 )]; their slots follow from faceDir
//               and k.  The head writes nbr[slot][vertex] (six arrays, only the slots of its mask), the mask and the corner key with plain stores.
//   iteration   kSmoothStep, one thread per vertex: its own d and those of the neighbours its mask names, 4 x int16 = one 8-byte load each; the clamp count
//               by a wave reduction and one atomic per wave.
//   output      kSmoothWrite, one thread per vertex, from the buffer the last iteration wrote: d as 3 x int32, the position, the mask.
//
// The arithmetic is smooth_rule.h, host-callable and checked exhaustively by tests/hip/smooth_host.hip.
#include "launch.h"
#include "smooth_rule.h"
#include "surface_weld.h"
#include "voxel_passes.h"

#define SB 256 // threads per workgroup

namespace
{
// keys / vals / rank1: the weld.  nbr: 6 arrays of nVertices entries, array s = the neighbour in slot s.  Entries of slots outside the mask stay unwritten and
// are never read.
__global__ void __launch_bounds__( SB ) kSmoothNeighbours( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ rank1, uint32_t nCorners,
														   uint32_t nVertices, const uint8_t* __restrict__ faceDir, const uint32_t* __restrict__ indices, uint32_t* __restrict__ nbr,
														   uint8_t* __restrict__ mask, uint64_t* __restrict__ vkey )
{
	const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( i >= nCorners ) return;
	const uint64_t key = keys[i];
	if( i > 0 && keys[i - 1] == key ) return; // not the head of its run
	const uint32_t r = rank1[i] - 1u;
	uint32_t m = 0;
	for( uint64_t j = i; j < nCorners && ( j == i || keys[j] == key ); j++ )
	{
		const uint32_t v = vals[j], f = v >> 2, k = v & 3u, d = faceDir[f];
		const uint32_t c0 = faceCorner( d, k );
#pragma unroll
		for( uint32_t step = 1; step < 4; step += 2 ) // the corners k + 1 and k - 1 of the quad
		{
			const uint32_t k1 = ( k + step ) & 3u, c1 = faceCorner( d, k1 );
			const uint32_t slot = smoothSlot( cornerX( c0 ), cornerY( c0 ), cornerZ( c0 ), cornerX( c1 ), cornerY( c1 ), cornerZ( c1 ) );
			nbr[(uint64_t)slot * nVertices + r] = indices[(uint64_t)f * 4 + k1];
			m |= 1u << slot;
		}
	}
	mask[r] = (uint8_t)m;
	vkey[r] = key;
}

// one Jacobi step with the weight w: out = the step of `in`.  All 64 lanes of a wave reach the reduction.
__global__ void __launch_bounds__( SB ) kSmoothStep( const short4* __restrict__ in, short4* __restrict__ out, const uint32_t* __restrict__ nbr, const uint8_t* __restrict__ mask,
													 uint32_t nVertices, int32_t w, int32_t limit, unsigned long long* __restrict__ clamped )
{
	const uint64_t r = (uint64_t)blockIdx.x * SB + threadIdx.x;
	uint32_t cnt = 0;
	if( r < nVertices )
	{
		const uint32_t m = mask[r];
		const short4 own = in[r];
		int32_t sx = 0, sy = 0, sz = 0;
#pragma unroll
		for( uint32_t s = 0; s < 6; s++ )
			if( ( m >> s ) & 1u )
			{
				const short4 q = in[nbr[(uint64_t)s * nVertices + r]];
				sx += q.x;
				sy += q.y;
				sz += q.z;
			}
		const int32_t n = __popc( m );
		short4 o;
		o.x = (short)smoothStep( own.x, sx, (int32_t)( ( m >> 1 ) & 1u ) - (int32_t)( m & 1u ), n, w, limit, &cnt );
		o.y = (short)smoothStep( own.y, sy, (int32_t)( ( m >> 3 ) & 1u ) - (int32_t)( ( m >> 2 ) & 1u ), n, w, limit, &cnt );
		o.z = (short)smoothStep( own.z, sz, (int32_t)( ( m >> 5 ) & 1u ) - (int32_t)( ( m >> 4 ) & 1u ), n, w, limit, &cnt );
		o.w = 0;
		out[r] = o;
	}
	waveAddInto( clamped, cnt );
}

// any output may be null
__global__ void __launch_bounds__( SB ) kSmoothWrite( const short4* __restrict__ d, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ vkey, uint32_t nVertices, f3 lower,
													  float dps, uint32_t gridRes, float* __restrict__ vertices, int32_t* __restrict__ displacements, uint8_t* __restrict__ neighbours )
{
	const uint64_t r = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( r >= nVertices ) return;
	const short4 v = d[r];
	if( displacements )
	{
		displacements[r * 3] = v.x;
		displacements[r * 3 + 1] = v.y;
		displacements[r * 3 + 2] = v.z;
	}
	if( neighbours ) neighbours[r] = mask[r];
	if( vertices )
	{
		const uint64_t key = vkey[r], R1 = (uint64_t)gridRes + 1ull; // the decode of kSurfaceWeld
		const uint64_t zy = key / R1;
		const uint32_t cx = (uint32_t)( key - zy * R1 ), cz = (uint32_t)( zy / R1 ), cy = (uint32_t)( zy - (uint64_t)cz * R1 );
		vertices[r * 3] = smoothPosition( cx, v.x, lower.x, dps );
		vertices[r * 3 + 1] = smoothPosition( cy, v.y, lower.y, dps );
		vertices[r * 3 + 2] = smoothPosition( cz, v.z, lower.z, dps );
	}
}
} // namespace

int surfaceSmooth( const SurfaceSource& s, const uint8_t* givenMasks, const SmoothRule& rule, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev,
				   uint32_t* indicesDev, float* verticesDev, int32_t* displacementsDev, uint8_t* neighboursDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, uint64_t* clampedOut,
				   hipStream_t st )
{
	const char* who = "mvrt_svo_surface_smooth";
	DevBuf masks, offs;
	uint64_t nFaces = 0;
	if( clampedOut ) *clampedOut = 0;
	if( surfaceScratchMasks( s, givenMasks, masks, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	if( nVerticesOut ) *nVerticesOut = 0;
	if( 4ull * nFaces >= ( 1ull << 32 ) )
	{
		mvrtSetError( "%s: the %llu faces of the surface have 2^32 corners or more, beyond the 32-bit indices of a welded mesh", who, (unsigned long long)nFaces );
		return 1;
	}
	const uint32_t nCorners = (uint32_t)( 4ull * nFaces );
	SurfaceWeld weld;
	if( nCorners )
	{
		if( surfaceScanOffsets( s, masks, offs, st ) ) return 1;
		DevBuf keysA, valsA;
		if( keysA.alloc( (uint64_t)nCorners * 8 ) || valsA.alloc( (uint64_t)nCorners * 4 ) ) return 1;
		if( surfaceLaunchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), nullptr, nullptr, nullptr, keysA.as<uint64_t>(), valsA.as<uint32_t>(), st ) ) return 1;
		if( surfaceBuildWeld( s, keysA, valsA, nCorners, &weld, st ) ) return 1;
	}
	const uint32_t nVertices = weld.nVertices;
	if( nVerticesOut ) *nVerticesOut = nVertices;
	if( !faceVoxelDev && !faceDirDev && !indicesDev && !verticesDev && !displacementsDev && !neighboursDev ) return 0; // the sizing call: no iteration
	if( ( faceVoxelDev || faceDirDev || indicesDev ) && faceCapacity < nFaces )
	{
		listingRefusal( who, "faceCapacity", "faces of the surface", faceCapacity, nFaces );
		return 1;
	}
	if( ( verticesDev || displacementsDev || neighboursDev ) && vertexCapacity < nVertices )
	{
		listingRefusal( who, "vertexCapacity", "vertices of the surface", vertexCapacity, nVertices );
		return 1;
	}
	if( nCorners == 0 ) return 0;

	// every allocation before the first store into a caller's array: faceDir and indices where the caller takes none, the table, the two displacement buffers
	DevBuf dirScratch, idxScratch, nbr, mask, vkey, dA, dB;
	Counters cnt;
	if( !faceDirDev && dirScratch.alloc( nFaces ) ) return 1;
	if( !indicesDev && idxScratch.alloc( (uint64_t)nCorners * 4 ) ) return 1;
	if( nbr.alloc( (uint64_t)nVertices * 24 ) || mask.alloc( nVertices ) || vkey.alloc( (uint64_t)nVertices * 8 ) || dA.alloc( (uint64_t)nVertices * 8 ) ) return 1;
	if( rule.iterations > 0 && dB.alloc( (uint64_t)nVertices * 8 ) ) return 1;
	if( cnt.init( 1, st ) ) return 1;
	uint8_t* faceDir = faceDirDev ? faceDirDev : dirScratch.as<uint8_t>();
	uint32_t* indices = indicesDev ? indicesDev : idxScratch.as<uint32_t>();
	if( surfaceLaunchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), faceVoxelDev, faceDir, nullptr, nullptr, nullptr, st ) ) return 1;
	if( surfaceWriteWeld( s, weld, indices, nullptr, st ) ) return 1;
	hipLaunchKernelGGL( kSmoothNeighbours, dim3( divUp( nCorners, SB ) ), dim3( SB ), 0, st, weld.keys.as<uint64_t>(), weld.vals.as<uint32_t>(), weld.rank1.as<uint32_t>(), nCorners, nVertices,
						faceDir, indices, nbr.as<uint32_t>(), mask.as<uint8_t>(), vkey.as<uint64_t>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipMemsetAsync( dA.p, 0, (uint64_t)nVertices * 8, st ) );
	short4 *from = dA.as<short4>(), *to = dB.as<short4>();
	const dim3 grid( divUp( nVertices, SB ) );
	for( int k = 0; k < rule.iterations; k++ )
	{
		hipLaunchKernelGGL( kSmoothStep, grid, dim3( SB ), 0, st, from, to, nbr.as<uint32_t>(), mask.as<uint8_t>(), nVertices, ( k & 1 ) ? rule.weightOdd : rule.weightEven, rule.limit,
							cnt.dev() );
		MVRT_HIP( hipGetLastError() );
		short4* t = from;
		from = to;
		to = t;
	}
	// `from` is what the last iteration wrote, for odd and even counts alike (dA itself for none)
	hipLaunchKernelGGL( kSmoothWrite, grid, dim3( SB ), 0, st, from, mask.as<uint8_t>(), vkey.as<uint64_t>(), nVertices, s.lower, s.dps, 1u << s.levels, verticesDev, displacementsDev,
						neighboursDev );
	MVRT_HIP( hipGetLastError() );
	unsigned long long clamped = 0;
	if( cnt.read( &clamped, 1, st ) ) return 1; // (waits: the scratch is released on return)
	if( clampedOut ) *clampedOut = clamped;
	return 0;
}
