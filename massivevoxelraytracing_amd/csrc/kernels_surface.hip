// kernels_surface.hip -- the exposed faces of the voxel set as a quad mesh (mvrt_svo_surface_masks / _quads / _mesh, mvrt.h), the GPU form of the
// reference voxelizer's "Save As Mesh" (voxMesh.cpp:111-219, voxelMeshWriter.hpp), which asks a sorted host list six times per voxel.
//
//   masks   one byte per voxel, bit d = the neighbour in direction d is empty.  Read from the sorted Morton codes of the build; a neighbour is looked up in the
//           cell index (SvoDev::cellBlocks / cellEntries) where the octree has one, else by binary search in the codes.  Both give the same bytes.
//           The _masked calls take a caller's bytes instead (kSurfaceGivenMasks copies them, without bits 6-7, and counts); everything behind the masks reads
//           the masks alone, never occupancy.
//   faces   exclusive scan of the popcounts (64-bit offsets), then the run expansion of voxel_passes.h: one workgroup per 256 voxels emits that group's faces,
//           one thread per face, so a wave writes 64 consecutive records.
//   weld    corner keys, then the SurfaceWeld record: radix sort of (key, face * 4 + k), head flags, inclusive scan = rank + 1; scatter of the ranks and decode of the heads.
//
// The codec, the searches and the host steps (exclusiveOffsets, sortPairsInto, rankHeads) are those of mvrt_common.h and voxel_passes.h; the four
// corners of a quad are emitQuadCorners here, for the unit faces and for the merged rectangles.
//
// Directions, corners and windings are the reference's (voxMesh.cpp:172-200); positions are lower + (float)c * dps, one multiply and one add, each rounded
// (this file is compiled without contraction like every other).
#include "launch.h"
#include "surface_weld.h"
#include "voxel_passes.h"

#define SB 256 // threads per workgroup, and voxels per workgroup of the emit kernel

namespace
{
// direction d (voxMesh.cpp:172-200): 0 = -Y, 1 = +Y, 2 = -Z, 3 = +X, 4 = +Z, 5 = -X
MVRT_DI uint32_t dirAxis( uint32_t d ) { return ( 0x020211u >> ( 4u * d ) ) & 3u; } // x = 0, y = 1, z = 2
MVRT_DI uint32_t dirPositive( uint32_t d ) { return ( 0x1Au >> d ) & 1u; }			 // +Y, +X, +Z

// mask of the voxels of one 2 x 2 x 2 cell (a cell code = a voxel code >> 3); 0 where the block or the cell holds none
MVRT_DI uint32_t cellMaskOf( const SurfaceSource& s, uint64_t cell )
{
	const uint32_t b = s.cellBlocks[cell >> s.cellBits];
	if( b == 0xFFFFFFFFu ) return 0u;
	return s.cellEntries[( (uint64_t)b << s.cellBits ) | ( (uint32_t)cell & ( ( 1u << s.cellBits ) - 1u ) )].y;
}
MVRT_DI bool codePresent( const uint64_t* __restrict__ morton, uint32_t n, uint64_t code ) // binary search in the sorted unique codes
{
	const uint64_t i = lowerBound( morton, 0, n, code );
	return i < n && morton[i] == code;
}
template <bool CELLS> MVRT_DI uint32_t exposureMask( const SurfaceSource& s, uint64_t c )
{
	const uint64_t codeBits = ( 1ull << ( 3u * s.levels ) ) - 1ull; // levels <= 21
	const uint32_t inCell = (uint32_t)c & 7u;
	const uint32_t own = CELLS ? cellMaskOf( s, c >> 3 ) : 0u;
	uint32_t m = 0;
#pragma unroll
	for( uint32_t d = 0; d < 6; d++ )
	{
		const uint32_t a = dirAxis( d ), pos = dirPositive( d );
		const uint64_t M = splitBy3( 0x1FFFFFu ) << a; // the bits of axis a in a Morton code
		bool present;
		if( CELLS && ( ( inCell >> a ) & 1u ) != pos ) // the neighbour shares this voxel's cell
			present = ( own >> ( inCell ^ ( 1u << a ) ) ) & 1u;
		else if( pos ? ( c & M & codeBits ) == ( M & codeBits ) : ( c & M ) == 0ull ) // outside [0, gridRes): empty, and no 21-bit wrap
			present = false;
		else
		{
			const uint64_t nc = ( ( pos ? ( c | ~M ) + 1ull : ( c & M ) - 1ull ) & M ) | ( c & ~M ); // +-1 on one axis of a Morton code
			present = CELLS ? ( ( cellMaskOf( s, nc >> 3 ) >> ( (uint32_t)nc & 7u ) ) & 1u ) != 0u : codePresent( s.morton, s.nVoxels, nc );
		}
		if( !present ) m |= 1u << d;
	}
	return m;
}

// two voxels per thread: one 16-byte load of the codes; nFaces by a wave reduction and one atomic per wave
template <bool CELLS> __global__ void __launch_bounds__( SB ) kSurfaceMasks( SurfaceSource s, uint8_t* __restrict__ masks, unsigned long long* __restrict__ nFaces )
{
	const uint64_t i = ( (uint64_t)blockIdx.x * SB + threadIdx.x ) * 2ull;
	uint32_t cnt = 0;
	if( i < s.nVoxels )
	{
		const bool two = i + 1 < s.nVoxels;
		uint64_t c0, c1 = 0;
		if( two )
		{
			const ulonglong2 v = *reinterpret_cast<const ulonglong2*>( s.morton + i );
			c0 = v.x;
			c1 = v.y;
		}
		else
			c0 = s.morton[i];
		const uint32_t m0 = exposureMask<CELLS>( s, c0 );
		const uint32_t m1 = two ? exposureMask<CELLS>( s, c1 ) : 0u;
		cnt = __popc( m0 ) + __popc( m1 );
		if( masks )
		{
			masks[i] = (uint8_t)m0;
			if( two ) masks[i + 1] = (uint8_t)m1;
		}
	}
	waveAddInto( nFaces, cnt );
}

// the caller's masks of the _masked calls into the scratch: bits 6 and 7 dropped, the set bits counted the same way
__global__ void __launch_bounds__( SB ) kSurfaceGivenMasks( const uint8_t* __restrict__ given, uint32_t n, uint8_t* __restrict__ masks, unsigned long long* __restrict__ nFaces )
{
	const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
	uint32_t cnt = 0;
	if( i < n )
	{
		const uint32_t m = given[i] & 0x3Fu;
		masks[i] = (uint8_t)m;
		cnt = __popc( m );
	}
	waveAddInto( nFaces, cnt );
}

struct PopcountOf // scan input: faces of voxel i
{
	__host__ __device__ uint64_t operator()( uint8_t m ) const { return popcount8( m ); }
};

// (the corner tables cornerX / cornerY / cornerZ / faceCorner: surface_weld.h)
// The four corners of quad f: direction d at voxel (x, y, z), a corner offset counting sx / sy / sz voxels on its axis (1, 1, 1: a unit face).  positions (12 floats
// per quad) and keys / vals (the weld's corner keys and f * 4 + k) may each be null.
template <bool V4>
MVRT_DI void emitQuadCorners( uint32_t x, uint32_t y, uint32_t z, uint32_t d, uint32_t sx, uint32_t sy, uint32_t sz, f3 lower, float dps, uint32_t gridRes, uint64_t f,
							  float* __restrict__ positions, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals )
{
	float p[12];
#pragma unroll
	for( uint32_t k = 0; k < 4; k++ )
	{
		const uint32_t cn = faceCorner( d, k );
		const uint32_t cx = x + cornerX( cn ) * sx, cy = y + cornerY( cn ) * sy, cz = z + cornerZ( cn ) * sz;
		p[k * 3] = lower.x + (float)cx * dps;
		p[k * 3 + 1] = lower.y + (float)cy * dps;
		p[k * 3 + 2] = lower.z + (float)cz * dps;
		if( keys )
		{
			const uint64_t R1 = (uint64_t)gridRes + 1ull;
			keys[f * 4 + k] = ( (uint64_t)cz * R1 + cy ) * R1 + cx;
			vals[f * 4 + k] = (uint32_t)( f * 4 + k );
		}
	}
	if( positions )
	{
		if( V4 )
		{
			float4* o = reinterpret_cast<float4*>( positions + f * 12 );
			o[0] = make_float4( p[0], p[1], p[2], p[3] );
			o[1] = make_float4( p[4], p[5], p[6], p[7] );
			o[2] = make_float4( p[8], p[9], p[10], p[11] );
		}
		else
		{
#pragma unroll
			for( int k = 0; k < 12; k++ ) positions[f * 12 + k] = p[k];
		}
	}
}

// One workgroup per SB voxels, the run expansion of voxel_passes.h: offs = n + 1 exclusive offsets (offs[n] = nFaces), the records are faces, a voxel's faces the set
// bits of its mask.  Any output may be null.  keys / vals: the weld's corner keys and face * 4 + k.
template <bool V4>
__global__ void __launch_bounds__( SB ) kSurfaceEmit( const uint64_t* __restrict__ morton, const uint8_t* __restrict__ masks, const uint64_t* __restrict__ offs, uint32_t n, f3 lower,
													  float dps, uint32_t gridRes, uint32_t* __restrict__ faceVoxel, uint8_t* __restrict__ faceDir, float* __restrict__ positions,
													  uint64_t* __restrict__ keys, uint32_t* __restrict__ vals )
{
	__shared__ uint32_t sOff[SB + 1];
	__shared__ uint8_t sMask[SB];
	__shared__ uint64_t sCode[SB];
	const uint64_t first = (uint64_t)blockIdx.x * SB;
	const uint64_t v = first + threadIdx.x;
	const uint64_t base = stageRunOffsets<SB>( offs, n, sOff ); // (relative offsets <= 6 * SB)
	sMask[threadIdx.x] = v < n ? masks[v] : (uint8_t)0;
	sCode[threadIdx.x] = v < n ? morton[v] : 0ull;
	__syncthreads();
	const uint32_t total = sOff[SB];
	for( uint32_t j = threadIdx.x; j < total; j += SB )
	{
		const uint32_t lo = findRun( sOff, SB, j );
		const uint32_t d = nthSetBit( sMask[lo], j - sOff[lo] );
		const uint64_t f = base + j;
		if( faceVoxel ) faceVoxel[f] = (uint32_t)( first + lo );
		if( faceDir ) faceDir[f] = (uint8_t)d;
		if( !positions && !keys ) continue;
		uint32_t x, y, z;
		mortonDecode( sCode[lo], x, y, z );
		emitQuadCorners<V4>( x, y, z, d, 1u, 1u, 1u, lower, dps, gridRes, f, positions, keys, vals );
	}
}

// (the head of a run of sorted corner keys, 1 where a key differs from the one before it: KeyHead, voxel_passes.h)
// sorted corners -> indices[face * 4 + k] = rank of the key, vertices[rank] = the key's position (written by the first corner of each run)
__global__ void __launch_bounds__( SB ) kSurfaceWeld( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ rank1, uint32_t nCorners,
													  f3 lower, float dps, uint32_t gridRes, uint32_t* __restrict__ indices, float* __restrict__ vertices )
{
	const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( i >= nCorners ) return;
	const uint32_t r = rank1[i] - 1u;
	if( indices ) indices[vals[i]] = r;
	const uint64_t key = keys[i];
	if( vertices && ( i == 0 || keys[i - 1] != key ) )
	{
		const uint64_t R1 = (uint64_t)gridRes + 1ull;
		const uint64_t zy = key / R1;
		const uint32_t cx = (uint32_t)( key - zy * R1 ), cz = (uint32_t)( zy / R1 ), cy = (uint32_t)( zy - (uint64_t)cz * R1 );
		vertices[(uint64_t)r * 3] = lower.x + (float)cx * dps;
		vertices[(uint64_t)r * 3 + 1] = lower.y + (float)cy * dps;
		vertices[(uint64_t)r * 3 + 2] = lower.z + (float)cz * dps;
	}
}
} // namespace

// ---- the host steps that kernels_smooth.hip shares (surface_weld.h) -------------------------------------------------------------------------------------------
int surfaceLaunchEmit( const SurfaceSource& s, const uint8_t* masks, const uint64_t* offs, uint32_t* faceVoxel, uint8_t* faceDir, float* positions, uint64_t* keys, uint32_t* vals,
				hipStream_t st )
{
	const dim3 grid( divUp( s.nVoxels, SB ) );
	const uint32_t R = 1u << s.levels;
	if( ( (uintptr_t)positions & 15u ) == 0 )
		hipLaunchKernelGGL( kSurfaceEmit<true>, grid, dim3( SB ), 0, st, s.morton, masks, offs, s.nVoxels, s.lower, s.dps, R, faceVoxel, faceDir, positions, keys, vals );
	else
		hipLaunchKernelGGL( kSurfaceEmit<false>, grid, dim3( SB ), 0, st, s.morton, masks, offs, s.nVoxels, s.lower, s.dps, R, faceVoxel, faceDir, positions, keys, vals );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// the masks kernel into `masks` (null = count only), or a caller's `given` masks copied there, and the sum of the popcounts, on the host when this returns
static int masksAndCount( const SurfaceSource& s, const uint8_t* given, uint8_t* masks, uint64_t* nFaces, hipStream_t st )
{
	Counters cnt;
	if( cnt.init( 1, st ) ) return 1;
	if( given )
	{
		hipLaunchKernelGGL( kSurfaceGivenMasks, dim3( divUp( s.nVoxels, SB ) ), dim3( SB ), 0, st, given, s.nVoxels, masks, cnt.dev() );
		MVRT_HIP( hipGetLastError() );
	}
	else if( launchSurfaceMasks( s, masks, cnt.dev(), st ) ) return 1;
	unsigned long long h = 0;
	if( cnt.read( &h, 1, st ) ) return 1;
	*nFaces = h;
	return 0;
}
// the same into scratch of n + 1 bytes, the last one 0 so that the scan below yields offs[n]
int surfaceScratchMasks( const SurfaceSource& s, const uint8_t* given, DevBuf& masks, uint64_t* nFaces, hipStream_t st )
{
	if( masks.alloc( (uint64_t)s.nVoxels + 1 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( masks.as<uint8_t>() + s.nVoxels, 0, 1, st ) );
	return masksAndCount( s, given, masks.as<uint8_t>(), nFaces, st );
}
int surfaceScanOffsets( const SurfaceSource& s, const DevBuf& masks, DevBuf& offs, hipStream_t st )
{
	hipcub::TransformInputIterator<uint64_t, PopcountOf, const uint8_t*> in( masks.as<uint8_t>(), PopcountOf() );
	return exclusiveOffsets<uint64_t>( in, (uint64_t)s.nVoxels + 1, offs, nullptr, st );
}

// (the weld of a list of quads, unit faces or merged rectangles: struct SurfaceWeld, surface_weld.h)
// from the keys and numbers of nCorners >= 1 corners (keysA / valsA are released): radix sort, head flags, inclusive scan.  The counts are on the host when this returns
int surfaceBuildWeld( const SurfaceSource& s, DevBuf& keysA, DevBuf& valsA, uint32_t nCorners, SurfaceWeld* w, hipStream_t st )
{
	int endBit = 3 * ( (int)s.levels + 1 ); // a key is below ( gridRes + 1 )^3 <= 2^( 3 * ( levels + 1 ) )
	if( endBit > 64 ) endBit = 64;
	if( sortPairsInto( keysA, valsA, nCorners, endBit, w->keys, w->vals, st ) ) return 1;
	if( rankHeadsOf( KeyHead{ w->keys.as<uint64_t>() }, nCorners, w->rank1, &w->nVertices, st ) ) return 1;
	w->nCorners = nCorners;
	return 0;
}
// indices[quad * 4 + k] and the vertices of a weld with corners; either may be null.  Not synchronised.
int surfaceWriteWeld( const SurfaceSource& s, const SurfaceWeld& w, uint32_t* indicesDev, float* verticesDev, hipStream_t st )
{
	if( !indicesDev && !verticesDev ) return 0;
	hipLaunchKernelGGL( kSurfaceWeld, dim3( divUp( w.nCorners, SB ) ), dim3( SB ), 0, st, w.keys.as<uint64_t>(), w.vals.as<uint32_t>(), w.rank1.as<uint32_t>(), w.nCorners, s.lower,
						s.dps, 1u << s.levels, indicesDev, verticesDev );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

int launchSurfaceMasks( const SurfaceSource& s, uint8_t* masks, unsigned long long* nFacesDev, hipStream_t st )
{
	const dim3 grid( divUp( s.nVoxels, 2 * SB ) );
	if( s.cellBlocks ) hipLaunchKernelGGL( kSurfaceMasks<true>, grid, dim3( SB ), 0, st, s, masks, nFacesDev );
	else hipLaunchKernelGGL( kSurfaceMasks<false>, grid, dim3( SB ), 0, st, s, masks, nFacesDev );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

int surfaceMasks( const SurfaceSource& s, uint8_t* masksDev, uint64_t* nFacesOut, hipStream_t st )
{
	uint64_t nFaces = 0;
	if( masksAndCount( s, nullptr, masksDev, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	return 0;
}

int surfaceQuads( const SurfaceSource& s, const uint8_t* givenMasks, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, uint64_t* nFacesOut, hipStream_t st )
{
	const char* who = givenMasks ? "mvrt_svo_surface_quads_masked" : "mvrt_svo_surface_quads";
	DevBuf masks, offs;
	uint64_t nFaces = 0;
	if( surfaceScratchMasks( s, givenMasks, masks, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	if( !faceVoxelDev && !faceDirDev && !positionsDev ) return 0; // the sizing call
	if( faceCapacity < nFaces )
	{
		listingRefusal( who, "faceCapacity", "faces of the surface", faceCapacity, nFaces );
		return 1;
	}
	if( surfaceScanOffsets( s, masks, offs, st ) ) return 1;
	if( surfaceLaunchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), faceVoxelDev, faceDirDev, positionsDev, nullptr, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int surfaceMesh( const SurfaceSource& s, const uint8_t* givenMasks, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev, float* verticesDev,
				 uint64_t* nFacesOut, uint64_t* nVerticesOut, hipStream_t st )
{
	const char* who = givenMasks ? "mvrt_svo_surface_mesh_masked" : "mvrt_svo_surface_mesh";
	DevBuf masks, offs;
	uint64_t nFaces = 0;
	if( surfaceScratchMasks( s, givenMasks, masks, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	if( nVerticesOut ) *nVerticesOut = 0;
	if( 4ull * nFaces >= ( 1ull << 32 ) )
	{
		mvrtSetError( "%s: the %llu faces of the surface have 2^32 corners or more, beyond the 32-bit indices of a welded mesh (use mvrt_svo_surface_quads)", who,
					  (unsigned long long)nFaces );
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
	if( !faceVoxelDev && !faceDirDev && !indicesDev && !verticesDev ) return 0; // the sizing call
	// (the capacities are looked at behind the sort: a refused call still returns BOTH counts, and the vertex count is the sort's result)
	if( ( faceVoxelDev || faceDirDev || indicesDev ) && faceCapacity < nFaces )
	{
		listingRefusal( who, "faceCapacity", "faces of the surface", faceCapacity, nFaces );
		return 1;
	}
	if( verticesDev && vertexCapacity < nVertices )
	{
		listingRefusal( who, "vertexCapacity", "vertices of the surface", vertexCapacity, nVertices );
		return 1;
	}
	if( nCorners == 0 ) return 0;
	if( ( faceVoxelDev || faceDirDev ) && surfaceLaunchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), faceVoxelDev, faceDirDev, nullptr, nullptr, nullptr, st ) ) return 1;
	if( surfaceWriteWeld( s, weld, indicesDev, verticesDev, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

// ---- merged rectangles (mvrt_svo_surface_merged; the rule is in mvrt.h, the passes in DESIGN.md 5.11) ----------------------------------------------------
// One direction at a time.  A face of direction d is the key p << 2L | v << L | u (L = levels bits per field: p the voxel's coordinate on the normal axis,
// (u, v) its coordinates on the two other axes, the lower-numbered axis u) with the value vIndex.  Sorted, the faces of a row (p, v) lie together by u:
// head flags end a run where u is not one higher IN THE SAME ROW or the attributes differ.  The runs, keyed p << 2L | u0 << L | v, are sorted again: runs that
// start at the same u0 lie together by v, and head flags end a stack where v is not one higher IN THE SAME COLUMN, du differs or the attributes differ.
// The heads of the second pass, in its order, are the rectangles of the direction in (p, u0, v0) order.
namespace
{
struct MergeRect // one rectangle of a direction, kept until every direction is counted
{
	uint32_t voxel, du, dv; // the anchor face's vIndex and the extent in faces
};

struct BitOf // scan input: 1 where voxel i has a face in direction d
{
	uint32_t d;
	__host__ __device__ uint32_t operator()( uint8_t m ) const { return ( (uint32_t)m >> d ) & 1u; }
};
struct FlagOf // scan input: a head flag
{
	__host__ __device__ uint32_t operator()( uint8_t f ) const { return f; }
};

// in-plane axes of normal axis a: x -> (y, z), y -> (x, z), z -> (x, y)
MVRT_DI uint32_t axisU( uint32_t a ) { return a == 0u ? 1u : 0u; }
MVRT_DI uint32_t axisV( uint32_t a ) { return a == 2u ? 1u : 2u; }
MVRT_DI bool sameAttribute( const uint2* __restrict__ attrs, uint32_t v0, uint32_t v1 ) // all 8 bytes, one 8-byte load each
{
	const uint2 a = attrs[v0], b = attrs[v1];
	return a.x == b.x && a.y == b.y;
}

// offs: n + 1 exclusive offsets of bit d.  The voxels with the bit write their record at their offset: the set lanes of a wave write consecutive records.
__global__ void __launch_bounds__( SB ) kMergeFaceKeys( const uint64_t* __restrict__ morton, const uint8_t* __restrict__ masks, const uint32_t* __restrict__ offs, uint32_t n, uint32_t d,
															uint32_t levels, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals )
{
	const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( i >= n || !( ( masks[i] >> d ) & 1u ) ) return;
	const uint64_t c = morton[i];
	const uint32_t xyz[3] = { compactBy3( c ), compactBy3( c >> 1 ), compactBy3( c >> 2 ) };
	const uint32_t a = dirAxis( d );
	const uint32_t o = offs[i];
	keys[o] = ( (uint64_t)xyz[a] << ( 2u * levels ) ) | ( (uint64_t)xyz[axisV( a )] << levels ) | xyz[axisU( a )];
	vals[o] = (uint32_t)i;
}

// step 1 on the sorted faces: flags[i] = 0 where face i continues the run of face i - 1.  "Same row, u one higher" is key == previous + 1 AND u != 0: the
// last face of a row and the first of the next differ by 1 too when the u field is full, which at `levels` bits per field it is at every gridRes.
__global__ void __launch_bounds__( SB ) kMergeRunHeads( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint2* __restrict__ attrs, uint32_t n, uint32_t levels,
															uint32_t anyAttribute, uint8_t* __restrict__ flags )
{
	const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( i >= n ) return;
	bool head = true;
	if( i > 0 )
	{
		const uint64_t k = keys[i];
		if( k == keys[i - 1] + 1ull && ( k & ( ( 1ull << levels ) - 1ull ) ) != 0ull ) head = !anyAttribute && !sameAttribute( attrs, vals[i], vals[i - 1] );
	}
	flags[i] = head ? 1 : 0;
}

// rank1 = inclusive scan of the flags: starts[r] = the r-th flagged entry, starts[count] = n
__global__ void __launch_bounds__( SB ) kMergeStarts( const uint8_t* __restrict__ flags, const uint32_t* __restrict__ rank1, uint32_t n, uint32_t* __restrict__ starts )
{
	const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( i >= n ) return;
	if( flags[i] ) starts[rank1[i] - 1u] = (uint32_t)i;
	if( i == n - 1u ) starts[rank1[i]] = n;
}

// run r = the faces [runStart[r], runStart[r + 1]) -> key p << 2L | u0 << L | v, value r
__global__ void __launch_bounds__( SB ) kMergeRunKeys( const uint64_t* __restrict__ faceKeys, const uint32_t* __restrict__ runStart, uint32_t nRuns, uint32_t levels,
														   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals )
{
	const uint64_t r = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( r >= nRuns ) return;
	const uint64_t k = faceKeys[runStart[r]];
	const uint64_t field = ( 1ull << levels ) - 1ull;
	keys[r] = ( k & ~( ( field << levels ) | field ) ) | ( ( k & field ) << levels ) | ( ( k >> levels ) & field );
	vals[r] = (uint32_t)r;
}

// step 2 on the sorted runs: flags[j] = 0 where run j stacks on run j - 1: same column and v one higher (the same trap as above), same du, same attribute
__global__ void __launch_bounds__( SB ) kMergeStackHeads( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ runStart,
															  const uint32_t* __restrict__ faceVoxel, const uint2* __restrict__ attrs, uint32_t nRuns, uint32_t levels, uint32_t anyAttribute,
															  uint8_t* __restrict__ flags )
{
	const uint64_t j = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( j >= nRuns ) return;
	bool head = true;
	if( j > 0 )
	{
		const uint64_t k = keys[j];
		if( k == keys[j - 1] + 1ull && ( k & ( ( 1ull << levels ) - 1ull ) ) != 0ull )
		{
			const uint32_t r = vals[j], q = vals[j - 1];
			const uint32_t i = runStart[r], h = runStart[q];
			head = runStart[r + 1] - i != runStart[q + 1] - h || ( !anyAttribute && !sameAttribute( attrs, faceVoxel[i], faceVoxel[h] ) );
		}
	}
	flags[j] = head ? 1 : 0;
}

// rectangle t of the direction = the sorted runs [rectStart[t], rectStart[t + 1])
__global__ void __launch_bounds__( SB ) kMergeRects( const uint32_t* __restrict__ rectStart, uint32_t nRects, const uint32_t* __restrict__ runOf, const uint32_t* __restrict__ runStart,
														 const uint32_t* __restrict__ faceVoxel, MergeRect* __restrict__ rects )
{
	const uint64_t t = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( t >= nRects ) return;
	const uint32_t j = rectStart[t];
	const uint32_t r = runOf[j];
	const uint32_t i = runStart[r];
	MergeRect o;
	o.voxel = faceVoxel[i];
	o.du = runStart[r + 1] - i;
	o.dv = rectStart[t + 1] - j;
	rects[t] = o;
}

// the rectangles of direction d at the running offset `base` of every output; any output may be null.  keys / vals: the weld's corner keys and rect * 4 + k.
template <bool V4>
__global__ void __launch_bounds__( SB ) kMergeEmit( const MergeRect* __restrict__ rects, uint32_t nRects, uint64_t base, uint32_t d, const uint64_t* __restrict__ morton, f3 lower, float dps,
														uint32_t gridRes, uint32_t* __restrict__ rectVoxel, uint8_t* __restrict__ rectDir, uint32_t* __restrict__ rectSize,
														float* __restrict__ positions, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals )
{
	const uint64_t t = (uint64_t)blockIdx.x * SB + threadIdx.x;
	if( t >= nRects ) return;
	const MergeRect r = rects[t];
	const uint64_t f = base + t;
	if( rectVoxel ) rectVoxel[f] = r.voxel;
	if( rectDir ) rectDir[f] = (uint8_t)d;
	if( rectSize )
	{
		rectSize[f * 2] = r.du;
		rectSize[f * 2 + 1] = r.dv;
	}
	if( !positions && !keys ) return;
	uint32_t x, y, z;
	mortonDecode( morton[r.voxel], x, y, z );
	const uint32_t a = dirAxis( d );
	uint32_t scale[3] = { 1u, 1u, 1u }; // a corner offset counts du on the u axis, dv on the v axis, 1 on the normal axis
	scale[axisU( a )] = r.du;
	scale[axisV( a )] = r.dv;
	emitQuadCorners<V4>( x, y, z, d, scale[0], scale[1], scale[2], lower, dps, gridRes, f, positions, keys, vals );
}

#define MERGE_LAUNCH( kernel, items, ... )                                                                     \
	do                                                                                                          \
	{                                                                                                           \
		hipLaunchKernelGGL( kernel, dim3( divUp( items, SB ) ), dim3( SB ), 0, st, __VA_ARGS__ );               \
		MVRT_HIP( hipGetLastError() );                                                                          \
	} while( 0 )

// n head flags -> starts (count + 1 entries, the last one n) and the count on the host
int startsOfHeads( const DevBuf& flags, uint32_t n, DevBuf& starts, uint32_t* count, hipStream_t st )
{
	DevBuf rank1;
	hipcub::TransformInputIterator<uint32_t, FlagOf, const uint8_t*> in( flags.as<uint8_t>(), FlagOf() );
	if( rankHeads( in, n, rank1, count, st ) ) return 1;
	if( starts.alloc( ( (uint64_t)*count + 1 ) * 4 ) ) return 1;
	MERGE_LAUNCH( kMergeStarts, n, flags.as<uint8_t>(), rank1.as<uint32_t>(), n, starts.as<uint32_t>() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (rank1 is released on return)
	return 0;
}

// the rectangles of direction d into `rects` (nRects of them; 0 leaves it empty)
int mergeDirection( const SurfaceSource& s, const uint8_t* masks /* n + 1, the last 0 */, uint32_t d, uint32_t anyAttribute, DevBuf& rects, uint32_t* nRects, hipStream_t st )
{
	*nRects = 0;
	const uint32_t n = s.nVoxels, L = s.levels;
	DevBuf faceKeys, faceVoxel; // the faces of this direction, sorted by (p, v, u)
	uint32_t nFaces = 0;
	{
		DevBuf offs, keysA, valsA;
		hipcub::TransformInputIterator<uint32_t, BitOf, const uint8_t*> in( masks, BitOf{ d } );
		if( exclusiveOffsets<uint32_t>( in, (uint64_t)n + 1, offs, &nFaces, st ) ) return 1;
		if( nFaces == 0 ) return 0;
		if( keysA.alloc( (uint64_t)nFaces * 8 ) || valsA.alloc( (uint64_t)nFaces * 4 ) ) return 1;
		MERGE_LAUNCH( kMergeFaceKeys, n, s.morton, masks, offs.as<uint32_t>(), n, d, L, keysA.as<uint64_t>(), valsA.as<uint32_t>() );
		if( sortPairsInto( keysA, valsA, nFaces, 3 * (int)L, faceKeys, faceVoxel, st ) ) return 1; // (waits: offs goes at scope end)
	}
	DevBuf flags, runStart;
	uint32_t nRuns = 0;
	if( flags.alloc( nFaces ) ) return 1;
	MERGE_LAUNCH( kMergeRunHeads, nFaces, faceKeys.as<uint64_t>(), faceVoxel.as<uint32_t>(), s.attrs, nFaces, L, anyAttribute, flags.as<uint8_t>() );
	if( startsOfHeads( flags, nFaces, runStart, &nRuns, st ) ) return 1;

	DevBuf runKeys, runOf; // the runs sorted by (p, u0, v): key and run number
	{
		DevBuf keysA, valsA;
		if( keysA.alloc( (uint64_t)nRuns * 8 ) || valsA.alloc( (uint64_t)nRuns * 4 ) ) return 1;
		MERGE_LAUNCH( kMergeRunKeys, nRuns, faceKeys.as<uint64_t>(), runStart.as<uint32_t>(), nRuns, L, keysA.as<uint64_t>(), valsA.as<uint32_t>() );
		if( sortPairsInto( keysA, valsA, nRuns, 3 * (int)L, runKeys, runOf, st ) ) return 1;
	}
	faceKeys.release();
	DevBuf rectStart;
	uint32_t count = 0;
	if( flags.alloc( nRuns ) ) return 1;
	MERGE_LAUNCH( kMergeStackHeads, nRuns, runKeys.as<uint64_t>(), runOf.as<uint32_t>(), runStart.as<uint32_t>(), faceVoxel.as<uint32_t>(), s.attrs, nRuns, L, anyAttribute,
				  flags.as<uint8_t>() );
	if( startsOfHeads( flags, nRuns, rectStart, &count, st ) ) return 1;
	if( rects.alloc( (uint64_t)count * sizeof( MergeRect ) ) ) return 1;
	MERGE_LAUNCH( kMergeRects, count, rectStart.as<uint32_t>(), count, runOf.as<uint32_t>(), runStart.as<uint32_t>(), faceVoxel.as<uint32_t>(), rects.as<MergeRect>() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	*nRects = count;
	return 0;
}
int launchMergeEmit( const SurfaceSource& s, const DevBuf* rects, const uint32_t* counts, uint32_t* rectVoxel, uint8_t* rectDir, uint32_t* rectSize, float* positions, uint64_t* keys,
					 uint32_t* vals, hipStream_t st )
{
	uint64_t base = 0;
	for( uint32_t d = 0; d < 6; base += counts[d], d++ )
	{
		if( counts[d] == 0 ) continue;
		if( ( (uintptr_t)positions & 15u ) == 0 )
			MERGE_LAUNCH( kMergeEmit<true>, counts[d], rects[d].as<MergeRect>(), counts[d], base, d, s.morton, s.lower, s.dps, 1u << s.levels, rectVoxel, rectDir, rectSize, positions, keys,
						  vals );
		else
			MERGE_LAUNCH( kMergeEmit<false>, counts[d], rects[d].as<MergeRect>(), counts[d], base, d, s.morton, s.lower, s.dps, 1u << s.levels, rectVoxel, rectDir, rectSize, positions, keys,
						  vals );
	}
	return 0;
}
} // namespace

int surfaceMerged( const SurfaceSource& s, const uint8_t* givenMasks, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev, uint8_t* rectDirDev, uint32_t* rectSizeDev,
				   float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut, uint64_t* nRectsOut, uint64_t* nVerticesOut, hipStream_t st )
{
	const char* who = givenMasks ? "mvrt_svo_surface_merged_masked" : "mvrt_svo_surface_merged";
	const bool welded = ( flags & 2u ) != 0; // MVRT_SURFACE_MERGE_WELD
	DevBuf rects[6];
	uint32_t counts[6];
	uint64_t nFaces = 0, nRects = 0;
	{
		DevBuf masks;
		if( surfaceScratchMasks( s, givenMasks, masks, &nFaces, st ) ) return 1;
		if( nFacesOut ) *nFacesOut = nFaces;
		if( nRectsOut ) *nRectsOut = 0;
		if( nVerticesOut ) *nVerticesOut = 0;
		for( uint32_t d = 0; d < 6; d++ )
		{
			if( mergeDirection( s, masks.as<uint8_t>(), d, flags & 1u /* MVRT_SURFACE_MERGE_ANY_ATTRIBUTE */, rects[d], &counts[d], st ) ) return 1;
			nRects += counts[d];
		}
	}
	if( nRectsOut ) *nRectsOut = nRects;
	SurfaceWeld weld;
	if( welded )
	{
		if( 4ull * nRects >= ( 1ull << 32 ) )
		{
			mvrtSetError( "%s: the %llu rectangles of the surface have 2^32 corners or more, beyond the 32-bit indices of a welded mesh (call without "
						  "MVRT_SURFACE_MERGE_WELD)", who,
						  (unsigned long long)nRects );
			return 1;
		}
		const uint32_t nCorners = (uint32_t)( 4ull * nRects );
		if( nCorners )
		{
			DevBuf keysA, valsA;
			if( keysA.alloc( (uint64_t)nCorners * 8 ) || valsA.alloc( (uint64_t)nCorners * 4 ) ) return 1;
			if( launchMergeEmit( s, rects, counts, nullptr, nullptr, nullptr, nullptr, keysA.as<uint64_t>(), valsA.as<uint32_t>(), st ) ) return 1;
			if( surfaceBuildWeld( s, keysA, valsA, nCorners, &weld, st ) ) return 1;
		}
		if( nVerticesOut ) *nVerticesOut = weld.nVertices;
	}
	const uint32_t nVertices = weld.nVertices;
	if( !rectVoxelDev && !rectDirDev && !rectSizeDev && !positionsDev && !indicesDev && !verticesDev ) return 0; // the sizing call
	if( ( rectVoxelDev || rectDirDev || rectSizeDev || positionsDev || indicesDev ) && rectCapacity < nRects )
	{
		listingRefusal( who, "rectCapacity", "rectangles of the surface", rectCapacity, nRects );
		return 1;
	}
	if( verticesDev && vertexCapacity < nVertices )
	{
		listingRefusal( who, "vertexCapacity", "vertices of the surface", vertexCapacity, nVertices );
		return 1;
	}
	if( nRects == 0 ) return 0;
	if( ( rectVoxelDev || rectDirDev || rectSizeDev || positionsDev ) && launchMergeEmit( s, rects, counts, rectVoxelDev, rectDirDev, rectSizeDev, positionsDev, nullptr, nullptr, st ) )
		return 1;
	if( surfaceWriteWeld( s, weld, indicesDev, verticesDev, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
