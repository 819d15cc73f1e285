// kernels_morph.hip -- dilation, erosion, closing and opening of the voxel set (mvrt_svo_dilation_cells / _erosion_voxels / _dilate / _erode / _close / _open, mvrt.h;
// DESIGN.md 5.18).  Every step is a pass over a sorted unique list of codes with its attributes; the levels are built once, by the caller, from the last list.
//
//   masks    per voxel the bits of its in-grid neighbours that are not in the list (morphEmptyMask, voxel_passes.h: one bounded search per neighbour).  An erosion
//            step keeps the voxels whose mask is 0; a dilation step adds the cells the set bits name.
//   dilate   run expansion over the popcounts of the masks: one record ( neighbour's code, source entry ) per set bit, 64 consecutive records per wave; the
//            records sorted by code (sortPairsInto), head flags, rankHeads: a new cell is one run of at most 26 records.  The head record of a run sums the six
//            channels of its sources and emits code, coarseAttrib( sums, count ) and count at the run's rank -- integer sums, so the order inside a run does not
//            matter.  The new cells and the old list, both sorted and disjoint, are merged by ranks: an entry goes to its own index plus lowerBound in the other
//            list.  The next step gets a sorted unique list; nothing is sorted but the records.
//   erode    an exclusive scan of the keep flags and one scatter (compactUnmasked).
// The merge, the compaction and the operator's frame (halves, unchanged test, emission scan) are the list steps of kernels_list.hip.  No floating point, no atomics.
#include "launch.h"
#include "voxel_passes.h"

#define MB 256 // threads per workgroup = items per workgroup of the run expansion

namespace
{
__global__ void __launch_bounds__( MB ) kMorphMasks( const uint64_t* __restrict__ codes, uint32_t n, uint32_t levels, int element, uint32_t* __restrict__ mask )
{
	const uint64_t i = (uint64_t)blockIdx.x * MB + threadIdx.x;
	if( i < n ) mask[i] = morphEmptyMask( codes, n, levels, element, codes[i] );
}
struct MaskLength // scan input: the records of voxel i (item n: 0)
{
	const uint32_t* mask;
	uint32_t n;
	__host__ __device__ uint64_t operator()( uint32_t i ) const { return i < n ? (uint64_t)__builtin_popcount( mask[i] ) : 0ull; }
};
// (the head of a run of sorted records, 1 where record i starts a new cell: KeyHead, voxel_passes.h)

// offs: the n + 1 exclusive sums of the popcounts.  gridDim.x = ceil( n / MB ); a workgroup without records writes nothing
__global__ void __launch_bounds__( MB ) kMorphEmit( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ mask, const uint64_t* __restrict__ offs, uint32_t n,
													 uint32_t levels, int element, uint64_t* __restrict__ keys, uint32_t* __restrict__ src )
{
	__shared__ uint32_t sOff[MB + 1];
	__shared__ uint64_t sCode[MB];
	__shared__ uint32_t sMask[MB];
	const uint64_t first = (uint64_t)blockIdx.x * MB, v = first + threadIdx.x;
	const uint64_t base = stageRunOffsets<MB>( offs, n, sOff ); // (relative offsets <= MB * 26)
	sCode[threadIdx.x] = v < n ? codes[v] : 0ull;
	sMask[threadIdx.x] = v < n ? mask[v] : 0u;
	__syncthreads();
	const uint32_t total = sOff[MB];
	for( uint32_t j = threadIdx.x; j < total; j += MB )
	{
		const uint32_t lo = findRun( sOff, MB, j );
		const uint32_t dir = nthSetBit( sMask[lo], j - sOff[lo] );
		uint32_t x, y, z;
		mortonDecode( sCode[lo], x, y, z );
		uint64_t c = 0ull;
		morphNeighbour( x, y, z, levels, element, dir, &c ); // (in the grid: the bit is set)
		keys[base + j] = c;
		src[base + j] = (uint32_t)( first + lo );
	}
}

// One thread per sorted record; the head of a run of equal keys (at most 26 records) emits the cell at its rank.  Every output may be null; attribs: two words per cell
__global__ void __launch_bounds__( MB ) kMorphCells( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ src, const uint32_t* __restrict__ rank1, uint32_t nRecords,
													  const uint2* __restrict__ attrs, uint64_t* __restrict__ codesOut, uint32_t* __restrict__ attribsOut,
													  uint32_t* __restrict__ countOut, uint32_t* __restrict__ xyzOut )
{
	const uint64_t p = (uint64_t)blockIdx.x * MB + threadIdx.x;
	if( p >= nRecords ) return;
	const uint64_t key = keys[p];
	if( p > 0 && keys[p - 1] == key ) return;
	uint64_t sums[6] = { 0ull, 0ull, 0ull, 0ull, 0ull, 0ull };
	uint32_t cnt = 0;
	for( uint64_t q = p; q < nRecords && keys[q] == key; q++ )
	{
		const uint2 a = attrs[src[q]];
		sums[0] += a.x & 0xFFu;
		sums[1] += ( a.x >> 8 ) & 0xFFu;
		sums[2] += ( a.x >> 16 ) & 0xFFu;
		sums[3] += a.y & 0xFFu;
		sums[4] += ( a.y >> 8 ) & 0xFFu;
		sums[5] += ( a.y >> 16 ) & 0xFFu;
		cnt++;
	}
	const uint64_t d = rank1[p] - 1u;
	const uint2 at = coarseAttrib( sums, cnt );
	if( codesOut ) codesOut[d] = key;
	if( attribsOut )
	{
		attribsOut[d * 2] = at.x;
		attribsOut[d * 2 + 1] = at.y;
	}
	if( countOut ) countOut[d] = cnt;
	if( xyzOut ) mortonDecode( key, xyzOut[d * 3], xyzOut[d * 3 + 1], xyzOut[d * 3 + 2] );
}

int launchMasks( const uint64_t* codes, uint32_t n, uint32_t levels, int element, DevBuf& mask, hipStream_t st )
{
	if( mask.alloc( (uint64_t)n * 4 ) ) return 1;
	hipLaunchKernelGGL( kMorphMasks, dim3( divUp( n, MB ) ), dim3( MB ), 0, st, codes, n, levels, element, mask.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// the new cells of one dilation step as sorted records: cell r is the run of records whose rank1 is r + 1.  Has waited for the stream.
struct Records
{
	DevBuf keys, src, rank1;
	uint32_t nRecords = 0, nCells = 0;
};
int dilationRecords( const char* who, const uint64_t* codes, uint32_t n, uint32_t levels, int element, Records* r, hipStream_t st )
{
	DevBuf mask, offs, keysA, srcA;
	if( launchMasks( codes, n, levels, element, mask, st ) ) return 1;
	uint64_t total = 0;
	if( exclusiveOffsetsOf<uint64_t>( MaskLength{ mask.as<uint32_t>(), n }, (uint64_t)n + 1, offs, &total, st ) ) return 1;
	if( total == 0 ) return 0; // a full grid
	if( total >= 0xFFFFFFFFull )
	{
		mvrtSetError( "%s: the %llu (voxel, empty neighbour) pairs of one step exceed the 32-bit index range", who, (unsigned long long)total );
		return 1;
	}
	if( keysA.alloc( total * 8 ) || srcA.alloc( total * 4 ) ) return 1;
	hipLaunchKernelGGL( kMorphEmit, dim3( divUp( n, MB ) ), dim3( MB ), 0, st, codes, mask.as<uint32_t>(), offs.as<uint64_t>(), n, levels, element, keysA.as<uint64_t>(),
						srcA.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	if( sortPairsInto( keysA, srcA, total, (int)( 3u * levels ), r->keys, r->src, st ) ) return 1;
	mask.release();
	offs.release();
	r->nRecords = (uint32_t)total;
	return rankHeadsOf( KeyHead{ r->keys.as<uint64_t>() }, total, r->rank1, &r->nCells, st );
}
int launchCells( const Records& r, const uint2* attrs, uint64_t* codes, uint32_t* attribs, uint32_t* count, uint32_t* xyz, hipStream_t st )
{
	hipLaunchKernelGGL( kMorphCells, dim3( divUp( r.nRecords, MB ) ), dim3( MB ), 0, st, r.keys.as<uint64_t>(), r.src.as<uint32_t>(), r.rank1.as<uint32_t>(), r.nRecords, attrs, codes,
						attribs, count, xyz );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// *changed = 0: the step adds (removes) nothing, and so would every further one
int dilateStep( const char* who, int step, VoxelList& l, uint32_t levels, int element, int* changed, hipStream_t st )
{
	*changed = 0;
	Records r;
	if( dilationRecords( who, l.codes, l.n, levels, element, &r, st ) ) return 1;
	if( r.nCells == 0 ) return 0;
	if( (uint64_t)l.n + r.nCells >= 0xFFFFFFFFull )
	{
		mvrtSetError( "%s: dilation step %d would make %llu voxels, beyond the 32-bit index range of the builder", who, step, (unsigned long long)l.n + r.nCells );
		return 1;
	}
	DevBuf newCodes, newAttrs, codes, attrs;
	if( newCodes.alloc( (uint64_t)r.nCells * 8 ) || newAttrs.alloc( (uint64_t)r.nCells * 8 ) ) return 1;
	if( launchCells( r, l.attrs, newCodes.as<uint64_t>(), newAttrs.as<uint32_t>(), nullptr, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) );
	const uint32_t nNew = r.nCells, nAll = l.n + nNew;
	r = Records();
	if( mergeLists( l.codes, l.attrs, l.n, newCodes.as<uint64_t>(), newAttrs.as<uint2>(), nNew, codes, attrs, st ) ) return 1; // (the inputs are released below)
	l.take( codes, attrs, nAll );
	*changed = 1;
	return 0;
}
int erodeStep( const char* who, int step, VoxelList& l, uint32_t levels, int element, int* changed, hipStream_t st )
{
	*changed = 0;
	DevBuf mask;
	SortedVoxels kept;
	if( launchMasks( l.codes, l.n, levels, element, mask, st ) ) return 1;
	if( compactUnmasked( l.codes, l.attrs, mask.as<uint32_t>(), l.n, false, kept, st ) ) return 1;
	if( kept.n == l.n ) return 0;
	if( kept.n == 0 )
	{
		mvrtSetError( "%s: erosion step %d would leave no voxel (it removes all %u)", who, step, l.n );
		return 1;
	}
	l.take( kept.codes, kept.attrs, kept.n );
	*changed = 1;
	return 0;
}
} // namespace

int morphDilationCells( const SurfaceSource& s, int element, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* countDev, uint64_t* nOut, hipStream_t st )
{
	Records r;
	if( dilationRecords( "mvrt_svo_dilation_cells", s.morton, s.nVoxels, s.levels, element, &r, st ) ) return 1;
	if( nOut ) *nOut = r.nCells;
	const int tail = listingTail( "mvrt_svo_dilation_cells", "capacity", "cells", !xyzDev && !attribsDev && !countDev, capacity, r.nCells );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	if( launchCells( r, s.attrs, nullptr, attribsDev, countDev, xyzDev, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int morphStepCodes( const char* who, const uint64_t* codes, const uint2* attrs, uint32_t n, uint32_t levels, int element, DevBuf& cellCodes, uint32_t* nCells, hipStream_t st )
{
	Records r;
	if( dilationRecords( who, codes, n, levels, element, &r, st ) ) return 1;
	*nCells = r.nCells;
	if( r.nCells == 0 ) return 0;
	if( cellCodes.alloc( (uint64_t)r.nCells * 8 ) || launchCells( r, attrs, cellCodes.as<uint64_t>(), nullptr, nullptr, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the records are released on return)
	return 0;
}

int morphErosionVoxels( const SurfaceSource& s, int element, uint64_t capacity, uint32_t* vIndexDev, uint64_t* nOut, hipStream_t st )
{
	DevBuf mask, offs;
	if( launchMasks( s.morton, s.nVoxels, s.levels, element, mask, st ) ) return 1;
	uint32_t nRemoved = 0;
	if( maskOffsets( mask.as<uint32_t>(), s.nVoxels, 1u, offs, &nRemoved, st ) ) return 1;
	if( nOut ) *nOut = nRemoved;
	const int tail = listingTail( "mvrt_svo_erosion_voxels", "capacity", "voxels", !vIndexDev, capacity, nRemoved );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's array is written by this launch alone, behind every allocation and check)
	if( launchCompactMasked( s.morton, s.attrs, mask.as<uint32_t>(), offs.as<uint32_t>(), s.nVoxels, 1u, nullptr, nullptr, vIndexDev, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int morphList( const char* who, const SurfaceSource& s, int element, int op, int steps, SortedVoxels& out, hipStream_t st )
{
	// a half: up to `steps` steps, ended by the first that changes nothing (so would every further one).  An idle first half still leaves the second its turn
	const uint32_t levels = s.levels;
	auto half = [=]( decltype( &dilateStep ) step ) {
		return [=]( VoxelList& l ) {
			for( int k = 1; k <= steps; k++ )
			{
				int changed = 0;
				if( step( who, k, l, levels, element, &changed, st ) ) return 1;
				if( !changed ) break;
			}
			return 0;
		};
	};
	return runListOperator( op, s, false, half( dilateStep ), half( erodeStep ), out, st );
}
