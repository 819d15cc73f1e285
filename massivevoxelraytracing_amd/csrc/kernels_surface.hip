// kernels_surface.hip -- the exposed faces of the voxel set as a quad mesh (mvrt_svo_surface_masks / _quads / _mesh, mvrt.h), the GPU form of the
// reference voxelizer's "Save As Mesh" (voxMesh.cpp:111-219, voxelMeshWriter.hpp), which asks a sorted host list six times per voxel.
//
//   masks   one byte per voxel, bit d = the neighbour in direction d is empty.  Read from the sorted Morton codes of the build; a neighbour is looked up in the
//           cell index (SvoDev::cellBlocks / cellEntries) where the octree has one, else by binary search in the codes.  Both give the same bytes.
//   faces   exclusive scan of the popcounts (64-bit offsets, rocPRIM), then one workgroup per 256 voxels emits that group's faces: the faces of a group are
//           one contiguous run of the output, every thread takes faces of the run and finds their voxel in the group's offsets (LDS), so a wave writes
//           64 consecutive records.
//   weld    corner keys, radix sort of (key, face * 4 + k), head flags, inclusive scan = rank + 1, scatter of the ranks and decode of the heads.
//
// Directions, corners and windings are the reference's (voxMesh.cpp:172-200); positions are lower + (float)c * dps, one multiply and one add, each rounded
// (this file is compiled without contraction like every other).
#include <hipcub/hipcub.hpp>

#include "launch.h"

#define WAVE 64
#define SB 256 // threads per workgroup, and voxels per workgroup of the emit kernel

namespace
{
constexpr uint64_t kDimMask = 0x1249249249249249ull; // the bits of x in a Morton code; y = << 1, z = << 2

MVRT_DI uint32_t compact3( uint64_t x )
{
	x &= kDimMask;
	x = ( x ^ ( x >> 2 ) ) & 0x10c30c30c30c30c3ull;
	x = ( x ^ ( x >> 4 ) ) & 0x100f00f00f00f00full;
	x = ( x ^ ( x >> 8 ) ) & 0x1f0000ff0000ffull;
	x = ( x ^ ( x >> 16 ) ) & 0x1f00000000ffffull;
	x = ( x ^ ( x >> 32 ) ) & 0x1fffffull;
	return (uint32_t)x;
}

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
	uint32_t lo = 0, hi = n;
	while( lo < hi )
	{
		const uint32_t mid = lo + ( ( hi - lo ) >> 1 );
		if( morton[mid] < code ) lo = mid + 1;
		else hi = mid;
	}
	return lo < n && morton[lo] == code;
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
		const uint64_t M = kDimMask << a;
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
	for( int o = WAVE / 2; o > 0; o >>= 1 ) cnt += __shfl_down( cnt, o, WAVE );
	if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 && cnt ) atomicAdd( nFaces, (unsigned long long)cnt );
}

struct PopcountOf // scan input: faces of voxel i
{
	__host__ __device__ uint64_t operator()( uint8_t m ) const
	{
		uint32_t v = m;
		v = ( v & 0x55u ) + ( ( v >> 1 ) & 0x55u );
		v = ( v & 0x33u ) + ( ( v >> 2 ) & 0x33u );
		return ( v & 0x0Fu ) + ( v >> 4 );
	}
};

// corner number -> offset (the reference's numbering): 0 (0,0,0) 1 (1,0,0) 2 (1,0,1) 3 (0,0,1) 4 (0,1,0) 5 (1,1,0) 6 (1,1,1) 7 (0,1,1)
MVRT_DI uint32_t cornerX( uint32_t c ) { return ( 0x66u >> c ) & 1u; }
MVRT_DI uint32_t cornerY( uint32_t c ) { return ( 0xF0u >> c ) & 1u; }
MVRT_DI uint32_t cornerZ( uint32_t c ) { return ( 0xCCu >> c ) & 1u; }
// face d, corner k -> corner number: -Y 3,2,1,0  +Y 4,5,6,7  -Z 0,1,5,4  +X 1,2,6,5  +Z 2,3,7,6  -X 3,0,4,7 (three bits each, corner 0 lowest)
MVRT_DI uint32_t faceCorner( uint32_t d, uint32_t k )
{
	const uint64_t lo = 03u | 02u << 3 | 01u << 6 | 00u << 9 | ( 04ull | 05u << 3 | 06u << 6 | 07u << 9 ) << 12 | ( 00ull | 01u << 3 | 05u << 6 | 04u << 9 ) << 24;
	const uint64_t hi = 01u | 02u << 3 | 06u << 6 | 05u << 9 | ( 02ull | 03u << 3 | 07u << 6 | 06u << 9 ) << 12 | ( 03ull | 00u << 3 | 04u << 6 | 07u << 9 ) << 24;
	return (uint32_t)( ( d < 3u ? lo >> ( 12u * d ) : hi >> ( 12u * ( d - 3u ) ) ) >> ( 3u * k ) ) & 7u;
}

// One workgroup per SB voxels.  offs: n + 1 exclusive offsets (offs[n] = nFaces).  The group's faces are the run [offs[first], offs[end]) of every output;
// thread t takes faces t, t + SB, ... of the run.  Any output may be null.  keys / vals: the weld's corner keys and face * 4 + k.
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
	const uint64_t base = offs[first];
	sOff[threadIdx.x] = (uint32_t)( offs[v < n ? v : n] - base ); // <= 6 * SB
	if( threadIdx.x == 0 ) sOff[SB] = (uint32_t)( offs[first + SB < n ? first + SB : n] - base );
	sMask[threadIdx.x] = v < n ? masks[v] : (uint8_t)0;
	sCode[threadIdx.x] = v < n ? morton[v] : 0ull;
	__syncthreads();
	const uint32_t total = sOff[SB];
	for( uint32_t j = threadIdx.x; j < total; j += SB )
	{
		// the last voxel of the group whose offset is <= j: voxels without faces repeat the offset of the next one and are passed over
		uint32_t lo = 0, hi = SB;
		while( hi - lo > 1 )
		{
			const uint32_t mid = ( lo + hi ) >> 1;
			if( sOff[mid] <= j ) lo = mid;
			else hi = mid;
		}
		uint32_t m = sMask[lo];
		for( uint32_t r = j - sOff[lo]; r > 0; r-- ) m &= m - 1u; // the ( j - offset )-th set bit
		const uint32_t d = (uint32_t)__ffs( (int)m ) - 1u;
		const uint64_t f = base + j;
		if( faceVoxel ) faceVoxel[f] = (uint32_t)( first + lo );
		if( faceDir ) faceDir[f] = (uint8_t)d;
		if( !positions && !keys ) continue;
		const uint64_t c = sCode[lo];
		const uint32_t x = compact3( c ), y = compact3( c >> 1 ), z = compact3( c >> 2 );
		float p[12];
#pragma unroll
		for( uint32_t k = 0; k < 4; k++ )
		{
			const uint32_t cn = faceCorner( d, k );
			const uint32_t cx = x + cornerX( cn ), cy = y + cornerY( cn ), cz = z + cornerZ( cn );
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
}

struct HeadOf // scan input: 1 where a sorted corner key differs from the one before it
{
	const uint64_t* keys;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return ( i == 0u || keys[i] != keys[i - 1u] ) ? 1u : 0u; }
};
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

int launchMasks( const SurfaceSource& s, uint8_t* masks, unsigned long long* nFacesDev, hipStream_t st )
{
	const dim3 grid( divUp( s.nVoxels, 2 * SB ) );
	if( s.cellBlocks ) hipLaunchKernelGGL( kSurfaceMasks<true>, grid, dim3( SB ), 0, st, s, masks, nFacesDev );
	else hipLaunchKernelGGL( kSurfaceMasks<false>, grid, dim3( SB ), 0, st, s, masks, nFacesDev );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
int launchEmit( const SurfaceSource& s, const uint8_t* masks, const uint64_t* offs, uint32_t* faceVoxel, uint8_t* faceDir, float* positions, uint64_t* keys, uint32_t* vals,
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

// the masks kernel into `masks` (null = count only) and the sum of the popcounts, on the host when this returns
int masksAndCount( const SurfaceSource& s, uint8_t* masks, uint64_t* nFaces, hipStream_t st )
{
	DevBuf cnt;
	if( cnt.alloc( 8 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( cnt.p, 0, 8, st ) );
	if( launchMasks( s, masks, cnt.as<unsigned long long>(), st ) ) return 1;
	unsigned long long h = 0;
	MVRT_HIP( hipMemcpyAsync( &h, cnt.p, 8, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	*nFaces = h;
	return 0;
}
// the same into scratch of n + 1 bytes, the last one 0 so that the scan below yields offs[n]
int scratchMasksAndCount( const SurfaceSource& s, DevBuf& masks, uint64_t* nFaces, hipStream_t st )
{
	if( masks.alloc( (uint64_t)s.nVoxels + 1 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( masks.as<uint8_t>() + s.nVoxels, 0, 1, st ) );
	return masksAndCount( s, masks.as<uint8_t>(), nFaces, st );
}
int scanOffsets( const SurfaceSource& s, const DevBuf& masks, DevBuf& offs, hipStream_t st )
{
	const uint64_t items = (uint64_t)s.nVoxels + 1;
	if( offs.alloc( items * 8 ) ) return 1;
	hipcub::TransformInputIterator<uint64_t, PopcountOf, const uint8_t*> in( masks.as<uint8_t>(), PopcountOf() );
	return withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) { return hipcub::DeviceScan::ExclusiveSum( tmp, tmpBytes, in, offs.as<uint64_t>(), items, st ); } );
}
} // namespace

int surfaceMasks( const SurfaceSource& s, uint8_t* masksDev, uint64_t* nFacesOut, hipStream_t st )
{
	uint64_t nFaces = 0;
	if( masksAndCount( s, masksDev, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	return 0;
}

int surfaceQuads( const SurfaceSource& s, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, uint64_t* nFacesOut, hipStream_t st )
{
	DevBuf masks, offs;
	uint64_t nFaces = 0;
	if( scratchMasksAndCount( s, masks, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	if( !faceVoxelDev && !faceDirDev && !positionsDev ) return 0; // the sizing call
	if( faceCapacity < nFaces )
	{
		mvrtSetError( "mvrt_svo_surface_quads: faceCapacity %llu is smaller than the %llu faces of the surface; nothing was written", (unsigned long long)faceCapacity,
					  (unsigned long long)nFaces );
		return 1;
	}
	if( scanOffsets( s, masks, offs, st ) ) return 1;
	if( launchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), faceVoxelDev, faceDirDev, positionsDev, nullptr, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int surfaceMesh( const SurfaceSource& s, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev, float* verticesDev,
				 uint64_t* nFacesOut, uint64_t* nVerticesOut, hipStream_t st )
{
	DevBuf masks, offs;
	uint64_t nFaces = 0;
	if( scratchMasksAndCount( s, masks, &nFaces, st ) ) return 1;
	if( nFacesOut ) *nFacesOut = nFaces;
	if( nVerticesOut ) *nVerticesOut = 0;
	if( 4ull * nFaces >= ( 1ull << 32 ) )
	{
		mvrtSetError( "mvrt_svo_surface_mesh: the %llu faces of the surface have 2^32 corners or more, beyond the 32-bit indices of a welded mesh (use mvrt_svo_surface_quads)",
					  (unsigned long long)nFaces );
		return 1;
	}
	const uint32_t nCorners = (uint32_t)( 4ull * nFaces );
	uint32_t nVertices = 0;
	DevBuf keysB, valsB, rank1;
	if( nCorners )
	{
		if( scanOffsets( s, masks, offs, st ) ) return 1;
		DevBuf keysA, valsA;
		if( keysA.alloc( (uint64_t)nCorners * 8 ) || valsA.alloc( (uint64_t)nCorners * 4 ) || keysB.alloc( (uint64_t)nCorners * 8 ) || valsB.alloc( (uint64_t)nCorners * 4 ) ) return 1;
		if( launchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), nullptr, nullptr, nullptr, keysA.as<uint64_t>(), valsA.as<uint32_t>(), st ) ) return 1;
		int endBit = 3 * ( (int)s.levels + 1 ); // a key is below ( gridRes + 1 )^3 <= 2^( 3 * ( levels + 1 ) )
		if( endBit > 64 ) endBit = 64;
		if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
				return hipcub::DeviceRadixSort::SortPairs( tmp, tmpBytes, keysA.as<uint64_t>(), keysB.as<uint64_t>(), valsA.as<uint32_t>(), valsB.as<uint32_t>(), (uint64_t)nCorners, 0,
														   endBit, st );
			} ) )
			return 1;
		keysA.release();
		valsA.release();
		if( rank1.alloc( (uint64_t)nCorners * 4 ) ) return 1;
		hipcub::CountingInputIterator<uint32_t> counting( 0u );
		hipcub::TransformInputIterator<uint32_t, HeadOf, hipcub::CountingInputIterator<uint32_t>> heads( counting, HeadOf{ keysB.as<uint64_t>() } );
		if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) { return hipcub::DeviceScan::InclusiveSum( tmp, tmpBytes, heads, rank1.as<uint32_t>(), (uint64_t)nCorners, st ); } ) )
			return 1;
		MVRT_HIP( hipMemcpyAsync( &nVertices, rank1.as<uint32_t>() + ( nCorners - 1 ), 4, hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
	}
	if( nVerticesOut ) *nVerticesOut = nVertices;
	if( !faceVoxelDev && !faceDirDev && !indicesDev && !verticesDev ) return 0; // the sizing call
	// (the capacities are looked at behind the sort: a refused call still returns BOTH counts, and the vertex count is the sort's result)
	if( ( faceVoxelDev || faceDirDev || indicesDev ) && faceCapacity < nFaces )
	{
		mvrtSetError( "mvrt_svo_surface_mesh: faceCapacity %llu is smaller than the %llu faces of the surface; nothing was written", (unsigned long long)faceCapacity,
					  (unsigned long long)nFaces );
		return 1;
	}
	if( verticesDev && vertexCapacity < nVertices )
	{
		mvrtSetError( "mvrt_svo_surface_mesh: vertexCapacity %llu is smaller than the %u vertices of the surface; nothing was written", (unsigned long long)vertexCapacity, nVertices );
		return 1;
	}
	if( nCorners == 0 ) return 0;
	if( ( faceVoxelDev || faceDirDev ) && launchEmit( s, masks.as<uint8_t>(), offs.as<uint64_t>(), faceVoxelDev, faceDirDev, nullptr, nullptr, nullptr, st ) ) return 1;
	if( indicesDev || verticesDev )
	{
		hipLaunchKernelGGL( kSurfaceWeld, dim3( divUp( nCorners, SB ) ), dim3( SB ), 0, st, keysB.as<uint64_t>(), valsB.as<uint32_t>(), rank1.as<uint32_t>(), nCorners, s.lower, s.dps,
							1u << s.levels, indicesDev, verticesDev );
		MVRT_HIP( hipGetLastError() );
	}
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
