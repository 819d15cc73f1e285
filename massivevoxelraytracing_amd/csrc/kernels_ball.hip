// kernels_ball.hip -- round offsets of the voxel set: the exact distance band, the depth of the voxels and dilation, erosion, closing and opening with the ball
// B( rho ) (mvrt_svo_distance_cells / _depth_voxels / _dilate_ball / _erode_ball / _close_ball / _open_ball, mvrt.h).  One ball is one operation on
// sorted unique lists of codes; the levels are built once, by the caller, from the last list.
//
//   band     seeds ( code, payload ) -> every in-grid cell within rho of a seed, sorted, with the packed key d2 << 32 | payload minimised.  |c - v|^2 is a sum over
//            the axes, so three passes do it, along x, then y, then z.  A pass is a run expansion (ballShiftRange: the shifts of an entry are one interval, clipped
//            to the grid and to d2 + s * s <= rho, since partial sums only grow), one record ( shifted code, key + s * s << 32 ) per shift, 64 consecutive records
//            per wave; the records sorted by code (sortPairsInto), head flags, rankHeads; the head of a run, at most 2 k + 1 records, keeps the minimum key.
//            Adding a constant to the distance field keeps the order of two keys, so the result is the lexicographic minimum ( d2, payload ) over all seeds.
//            With a payload the sort carries the record's index and the keys stay where they were written; without one it carries d2 itself.
//   dilate   seeds = the voxels with an empty in-grid face neighbour (the nearest voxel of an empty cell is one of them), payload = vIndex.  The band minus the
//            cells of the set (one search each), scanned and scattered: code, d2, nearest voxel and its attribute with both alpha bytes 255.
//   erode    seeds = the cells of one FACES dilation step (the nearest empty cell of a voxel is one of them; morphStepCodes, kernels_morph.hip), no payload.  Every
//            voxel looks itself up in the band: found = its depth is <= rho.  The erosion's scan and scatter follow (compactUnmasked, kernels_list.hip).
// No floating point, no atomics.
#include "launch.h"
#include "voxel_passes.h"

#define BB 256 // threads per workgroup = items per workgroup of the run expansion

namespace
{
thread_local BallStats g_ballStats;

struct BandLength // scan input: the records of entry i in the pass along `axis` (item n: 0)
{
	const uint64_t *codes, *keys;
	uint32_t n, levels, axis, rho;
	__host__ __device__ uint64_t operator()( uint32_t i ) const
	{
		int32_t first;
		return i < n ? (uint64_t)ballShiftRange( ballAxisCoord( codes[i], axis ), levels, ballKeyDist2( keys[i] ), rho, &first ) : 0ull;
	}
};
// (the head of a run of sorted records: KeyHead, voxel_passes.h; the scans of the flags: maskOffsets with removed = 1, kernels_list.hip)

// offs: the n + 1 exclusive sums of BandLength.  gridDim.x = ceil( n / BB ).  recKeys != null: the record's key goes there and the sort carries its index;
// null: the sort carries d2
__global__ void __launch_bounds__( BB ) kBandEmit( const uint64_t* __restrict__ codes, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ offs, uint32_t n,
													uint32_t levels, uint32_t axis, uint32_t rho, uint64_t* __restrict__ recCodes, uint64_t* __restrict__ recKeys,
													uint32_t* __restrict__ recVals )
{
	__shared__ uint32_t sOff[BB + 1];
	__shared__ uint64_t sCode[BB], sKey[BB];
	__shared__ int32_t sFirst[BB];
	const uint64_t v = (uint64_t)blockIdx.x * BB + threadIdx.x;
	const uint64_t base = stageRunOffsets<BB>( offs, n, sOff ); // (relative offsets <= BB * 65)
	const uint64_t code = v < n ? codes[v] : 0ull, key = v < n ? keys[v] : 0ull;
	int32_t first = 0;
	if( v < n ) ballShiftRange( ballAxisCoord( code, axis ), levels, ballKeyDist2( key ), rho, &first );
	sCode[threadIdx.x] = code;
	sKey[threadIdx.x] = key;
	sFirst[threadIdx.x] = first;
	__syncthreads();
	const uint32_t total = sOff[BB];
	for( uint32_t j = threadIdx.x; j < total; j += BB )
	{
		const uint32_t e = findRun( sOff, BB, j );
		const int32_t s = sFirst[e] + (int32_t)( j - sOff[e] );
		uint64_t c = 0ull;
		ballShifted( sCode[e], levels, axis, s, &c ); // (in the grid: ballShiftRange clipped the interval)
		const uint64_t k = ballShiftKey( sKey[e], s );
		recCodes[base + j] = c;
		if( recKeys )
		{
			recKeys[base + j] = k;
			recVals[base + j] = (uint32_t)( base + j );
		}
		else recVals[base + j] = ballKeyDist2( k );
	}
}

// One thread per sorted record; the head of a run of equal codes (at most 65 records) emits the cell and its smallest key at its rank
__global__ void __launch_bounds__( BB ) kBandHeads( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ vals, const uint64_t* __restrict__ recKeys,
													 const uint32_t* __restrict__ rank1, uint32_t nRecords, uint64_t* __restrict__ codesOut, uint64_t* __restrict__ keysOut )
{
	const uint64_t p = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( p >= nRecords ) return;
	const uint64_t code = codes[p];
	if( p > 0 && codes[p - 1] == code ) return;
	uint64_t best = ~0ull;
	for( uint64_t q = p; q < nRecords && codes[q] == code; q++ )
	{
		const uint64_t k = recKeys ? recKeys[vals[q]] : ballKey( vals[q], 0u );
		best = k < best ? k : best;
	}
	const uint64_t d = rank1[p] - 1u;
	codesOut[d] = code;
	keysOut[d] = best;
}

__global__ void __launch_bounds__( BB ) kBallSeedFlags( const uint64_t* __restrict__ codes, uint32_t n, uint32_t levels, uint32_t* __restrict__ flag )
{
	const uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( i < n ) flag[i] = morphEmptyMask( codes, n, levels, 0, codes[i] ) != 0u ? 1u : 0u;
}
// offs: the exclusive sums of the flags.  The flagged voxels as seeds: their code and the key ( 0, vIndex )
__global__ void __launch_bounds__( BB ) kBallSeeds( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ offs, uint32_t n,
													 uint64_t* __restrict__ seedCodes, uint64_t* __restrict__ seedKeys )
{
	const uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( i >= n || flag[i] == 0u ) return;
	seedCodes[offs[i]] = codes[i];
	seedKeys[offs[i]] = ballKey( 0u, (uint32_t)i );
}
__global__ void __launch_bounds__( BB ) kBallOutside( const uint64_t* __restrict__ band, uint32_t nBand, const uint64_t* __restrict__ codes, uint32_t n, uint32_t* __restrict__ flag )
{
	const uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( i < nBand ) flag[i] = codePresentIn( codes, n, band[i] ) ? 0u : 1u;
}
// offs: the exclusive sums of the flags.  The flagged cells of the band, in order; any output may be null.  attribs: two words per cell
__global__ void __launch_bounds__( BB ) kBallCells( const uint64_t* __restrict__ band, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag,
													 const uint32_t* __restrict__ offs, uint32_t nBand, const uint2* __restrict__ attrs, uint64_t* __restrict__ codesOut,
													 uint32_t* __restrict__ xyzOut, uint32_t* __restrict__ dist2Out, uint32_t* __restrict__ nearestOut, uint32_t* __restrict__ attribsOut )
{
	const uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( i >= nBand || flag[i] == 0u ) return;
	const uint64_t d = offs[i], key = keys[i];
	const uint32_t near = ballKeyPayload( key );
	if( codesOut ) codesOut[d] = band[i];
	if( xyzOut ) mortonDecode( band[i], xyzOut[d * 3], xyzOut[d * 3 + 1], xyzOut[d * 3 + 2] );
	if( dist2Out ) dist2Out[d] = ballKeyDist2( key );
	if( nearestOut ) nearestOut[d] = near;
	if( attribsOut )
	{
		const uint2 a = attrs[near];
		attribsOut[d * 2] = a.x | 0xFF000000u; // (the rule of MVRT_VOXEL_SET: both alpha bytes are stored as 255)
		attribsOut[d * 2 + 1] = a.y | 0xFF000000u;
	}
}
// depth[i] = the squared distance the band holds for voxel i, 0 where the band does not hold it (a voxel is no seed, so a distance is at least 1)
__global__ void __launch_bounds__( BB ) kBallDepth( const uint64_t* __restrict__ codes, uint32_t n, const uint64_t* __restrict__ band, const uint64_t* __restrict__ keys,
													 uint32_t nBand, uint32_t* __restrict__ depth )
{
	const uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( i >= n ) return;
	const uint64_t j = codeIndexIn( band, nBand, codes[i] );
	depth[i] = j < nBand ? ballKeyDist2( keys[j] ) : 0u;
}
// offs: the exclusive sums of depth != 0.  Either output may be null
__global__ void __launch_bounds__( BB ) kBallDepthList( const uint32_t* __restrict__ depth, const uint32_t* __restrict__ offs, uint32_t n, uint32_t* __restrict__ vIndexOut,
														 uint32_t* __restrict__ depth2Out )
{
	const uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x;
	if( i >= n || depth[i] == 0u ) return;
	if( vIndexOut ) vIndexOut[offs[i]] = (uint32_t)i;
	if( depth2Out ) depth2Out[offs[i]] = depth[i];
}

// The band of n >= 1 seeds (both arrays are taken over).  payload: the low words of the keys matter.  Has waited for the stream
struct Band
{
	DevBuf codes, keys;
	uint32_t n = 0;
};
int distanceBand( const char* who, DevBuf& seedCodes, DevBuf& seedKeys, uint32_t nSeeds, uint32_t levels, uint32_t rho, bool payload, Band* b, hipStream_t st )
{
	static const char* const axisName[3] = { "x", "y", "z" };
	b->codes = std::move( seedCodes );
	b->keys = std::move( seedKeys );
	b->n = nSeeds;
	g_ballStats = BallStats();
	g_ballStats.seeds = nSeeds;
	for( uint32_t axis = 0; axis < 3; axis++ )
	{
		DevBuf offs, recCodes, recKeys, recVals, sortedCodes, sortedVals, rank1, outCodes, outKeys;
		const uint32_t n = b->n;
		uint64_t total = 0;
		if( exclusiveOffsetsOf<uint64_t>( BandLength{ b->codes.as<uint64_t>(), b->keys.as<uint64_t>(), n, levels, axis, rho }, (uint64_t)n + 1, offs, &total, st ) ) return 1;
		g_ballStats.records[axis] = total;
		if( total >= 0xFFFFFFFFull )
		{
			mvrtSetError( "%s: the %llu records of the pass along %s exceed the 32-bit index range", who, (unsigned long long)total, axisName[axis] );
			return 1;
		}
		if( recCodes.alloc( total * 8 ) || recVals.alloc( total * 4 ) || ( payload && recKeys.alloc( total * 8 ) ) ) return 1;
		hipLaunchKernelGGL( kBandEmit, dim3( divUp( n, BB ) ), dim3( BB ), 0, st, b->codes.as<uint64_t>(), b->keys.as<uint64_t>(), offs.as<uint64_t>(), n, levels, axis, rho,
							recCodes.as<uint64_t>(), recKeys.as<uint64_t>(), recVals.as<uint32_t>() );
		MVRT_HIP( hipGetLastError() );
		if( sortPairsInto( recCodes, recVals, total, (int)( 3u * levels ), sortedCodes, sortedVals, st ) ) return 1;
		offs.release();
		uint32_t nCells = 0;
		if( rankHeadsOf( KeyHead{ sortedCodes.as<uint64_t>() }, total, rank1, &nCells, st ) ) return 1;
		if( outCodes.alloc( (uint64_t)nCells * 8 ) || outKeys.alloc( (uint64_t)nCells * 8 ) ) return 1;
		hipLaunchKernelGGL( kBandHeads, dim3( divUp( total, BB ) ), dim3( BB ), 0, st, sortedCodes.as<uint64_t>(), sortedVals.as<uint32_t>(), recKeys.as<uint64_t>(), rank1.as<uint32_t>(),
							(uint32_t)total, outCodes.as<uint64_t>(), outKeys.as<uint64_t>() );
		MVRT_HIP( hipGetLastError() );
		MVRT_HIP( hipStreamSynchronize( st ) ); // (the records are released at the end of the turn)
		b->codes = std::move( outCodes );
		b->keys = std::move( outKeys );
		b->n = nCells;
	}
	g_ballStats.cells = b->n;
	return 0;
}

// the cells D_rho( A ) \ A of a list: the band of its seeds with a flag on the cells outside the list and the exclusive sums of the flags.  nNew == 0 (a full grid
// among the reasons): the arrays are not to be read.  Has waited for the stream
struct NewCells
{
	Band band;
	DevBuf flag, offs;
	uint32_t nNew = 0;
};
int dilationBand( const char* who, const uint64_t* codes, uint32_t n, uint32_t levels, uint32_t rho, NewCells* c, hipStream_t st )
{
	DevBuf seedFlag, seedOffs, seedCodes, seedKeys;
	if( seedFlag.alloc( (uint64_t)n * 4 ) ) return 1;
	hipLaunchKernelGGL( kBallSeedFlags, dim3( divUp( n, BB ) ), dim3( BB ), 0, st, codes, n, levels, seedFlag.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	uint32_t nSeeds = 0;
	if( maskOffsets( seedFlag.as<uint32_t>(), n, 1u, seedOffs, &nSeeds, st ) ) return 1;
	if( nSeeds == 0 ) return 0; // a full grid
	if( seedCodes.alloc( (uint64_t)nSeeds * 8 ) || seedKeys.alloc( (uint64_t)nSeeds * 8 ) ) return 1;
	hipLaunchKernelGGL( kBallSeeds, dim3( divUp( n, BB ) ), dim3( BB ), 0, st, codes, seedFlag.as<uint32_t>(), seedOffs.as<uint32_t>(), n, seedCodes.as<uint64_t>(),
						seedKeys.as<uint64_t>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) );
	seedFlag.release();
	seedOffs.release();
	if( distanceBand( who, seedCodes, seedKeys, nSeeds, levels, rho, true, &c->band, st ) ) return 1;
	const uint32_t nBand = c->band.n;
	if( c->flag.alloc( (uint64_t)nBand * 4 ) ) return 1;
	hipLaunchKernelGGL( kBallOutside, dim3( divUp( nBand, BB ) ), dim3( BB ), 0, st, c->band.codes.as<uint64_t>(), nBand, codes, n, c->flag.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	return maskOffsets( c->flag.as<uint32_t>(), nBand, 1u, c->offs, &c->nNew, st );
}
int launchNewCells( const NewCells& c, const uint2* attrs, uint64_t* codes, uint32_t* xyz, uint32_t* dist2, uint32_t* nearest, uint32_t* attribs, hipStream_t st )
{
	hipLaunchKernelGGL( kBallCells, dim3( divUp( c.band.n, BB ) ), dim3( BB ), 0, st, c.band.codes.as<uint64_t>(), c.band.keys.as<uint64_t>(), c.flag.as<uint32_t>(),
						c.offs.as<uint32_t>(), c.band.n, attrs, codes, xyz, dist2, nearest, attribs );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// depth (allocated here): per voxel of a list its squared depth where that is <= rho, else 0; offs: the exclusive sums of depth != 0, *nShallow of them.
// *nShallow == 0 (a full grid among the reasons): the arrays are not to be read.  Has waited for the stream
int depthBand( const char* who, const uint64_t* codes, const uint2* attrs, uint32_t n, uint32_t levels, uint32_t rho, DevBuf& depth, DevBuf& offs, uint32_t* nShallow, hipStream_t st )
{
	*nShallow = 0;
	DevBuf seedCodes, seedKeys;
	uint32_t nSeeds = 0;
	if( morphStepCodes( who, codes, attrs, n, levels, 0, seedCodes, &nSeeds, st ) ) return 1;
	if( nSeeds == 0 ) return 0; // a full grid: every depth is infinite
	if( seedKeys.alloc( (uint64_t)nSeeds * 8 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( seedKeys.p, 0, (uint64_t)nSeeds * 8, st ) );
	Band band;
	if( distanceBand( who, seedCodes, seedKeys, nSeeds, levels, rho, false, &band, st ) ) return 1;
	if( depth.alloc( (uint64_t)n * 4 ) ) return 1;
	hipLaunchKernelGGL( kBallDepth, dim3( divUp( n, BB ) ), dim3( BB ), 0, st, codes, n, band.codes.as<uint64_t>(), band.keys.as<uint64_t>(), band.n, depth.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	return maskOffsets( depth.as<uint32_t>(), n, 1u, offs, nShallow, st ); // (has waited: the band is released on return)
}

int dilateHalf( const char* who, VoxelList& l, uint32_t levels, uint32_t rho, hipStream_t st )
{
	DevBuf newCodes, newAttrs, codes, attrs;
	uint32_t nNew = 0;
	{
		NewCells c;
		if( dilationBand( who, l.codes, l.n, levels, rho, &c, st ) ) return 1;
		if( c.nNew == 0 ) return 0;
		if( (uint64_t)l.n + c.nNew >= 0xFFFFFFFFull )
		{
			mvrtSetError( "%s: the dilation would make %llu voxels, beyond the 32-bit index range of the builder", who, (unsigned long long)l.n + c.nNew );
			return 1;
		}
		nNew = c.nNew;
		if( newCodes.alloc( (uint64_t)nNew * 8 ) || newAttrs.alloc( (uint64_t)nNew * 8 ) ) return 1;
		if( launchNewCells( c, l.attrs, newCodes.as<uint64_t>(), nullptr, nullptr, nullptr, newAttrs.as<uint32_t>(), st ) ) return 1;
		MVRT_HIP( hipStreamSynchronize( st ) ); // (the band is released here)
	}
	if( mergeLists( l.codes, l.attrs, l.n, newCodes.as<uint64_t>(), newAttrs.as<uint2>(), nNew, codes, attrs, st ) ) return 1;
	l.take( codes, attrs, l.n + nNew );
	return 0;
}
int erodeHalf( const char* who, VoxelList& l, uint32_t levels, uint32_t rho, hipStream_t st )
{
	DevBuf depth, offs;
	SortedVoxels kept;
	uint32_t nShallow = 0;
	if( depthBand( who, l.codes, l.attrs, l.n, levels, rho, depth, offs, &nShallow, st ) ) return 1;
	if( nShallow == 0 ) return 0;
	if( nShallow == l.n )
	{
		mvrtSetError( "%s: the erosion would leave no voxel (it removes all %u)", who, l.n );
		return 1;
	}
	offs.release();
	if( compactUnmasked( l.codes, l.attrs, depth.as<uint32_t>(), l.n, true, kept, st ) ) return 1;
	l.take( kept.codes, kept.attrs, kept.n );
	return 0;
}
} // namespace

BallStats ballLastStats() { return g_ballStats; }

int ballDistanceCells( const SurfaceSource& s, uint32_t radius2, uint64_t capacity, uint32_t* xyzDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, uint64_t* nOut,
					   hipStream_t st )
{
	NewCells c;
	if( dilationBand( "mvrt_svo_distance_cells", s.morton, s.nVoxels, s.levels, radius2, &c, st ) ) return 1;
	if( nOut ) *nOut = c.nNew;
	const int tail = listingTail( "mvrt_svo_distance_cells", "capacity", "cells", !xyzDev && !dist2Dev && !nearestDev && !attribsDev, capacity, c.nNew );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	if( launchNewCells( c, s.attrs, nullptr, xyzDev, dist2Dev, nearestDev, attribsDev, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int ballDepthVoxels( const SurfaceSource& s, uint32_t radius2, uint64_t capacity, uint32_t* vIndexDev, uint32_t* depth2Dev, uint64_t* nOut, hipStream_t st )
{
	DevBuf depth, offs;
	uint32_t nShallow = 0;
	if( depthBand( "mvrt_svo_depth_voxels", s.morton, s.attrs, s.nVoxels, s.levels, radius2, depth, offs, &nShallow, st ) ) return 1;
	if( nOut ) *nOut = nShallow;
	const int tail = listingTail( "mvrt_svo_depth_voxels", "capacity", "voxels", !vIndexDev && !depth2Dev, capacity, nShallow );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	hipLaunchKernelGGL( kBallDepthList, dim3( divUp( s.nVoxels, BB ) ), dim3( BB ), 0, st, depth.as<uint32_t>(), offs.as<uint32_t>(), s.nVoxels, vIndexDev, depth2Dev );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int ballList( const char* who, const SurfaceSource& s, uint32_t radius2, int op, SortedVoxels& out, hipStream_t st )
{
	// one dilation, one erosion or both; a first half that changes nothing leaves nothing to the second
	const uint32_t levels = s.levels;
	return runListOperator(
		op, s, true, [=]( VoxelList& l ) { return dilateHalf( who, l, levels, radius2, st ); }, [=]( VoxelList& l ) { return erodeHalf( who, l, levels, radius2, st ); }, out, st );
}
