// kernels_nearest.hip -- the nearest voxel of every enclosed empty cell, without a radius (mvrt_svo_enclosed_nearest / mvrt_svo_fill_enclosed_nearest, mvrt.h;
// DESIGN.md 5.23).  The cells are those of kernels_fill.hip, whose classification (rows, gaps, unions, flatten, cell offsets) is run as it is.
//
//   lemma    for an enclosed cell c and a voxel v nearest to it, every cell of the path v -> (x, vy, vz) -> (x, y, vz) -> c is enclosed, and along an axis a maximal
//            run of enclosed cells, a gap, has a voxel at either end.  So three passes, along x, then y, then z, each minimising the packed key
//            ( d2 << 32 | vIndex ) of a cell over its own gap and the gap's two end voxels, give the exact ( d2, near ) of mvrt_svo_distance_cells.
//   pass x   the run expansion of the fill's emit: the enclosed x-gaps are the classified gaps.  One thread per gap finds the vIndex of its two end voxels (one
//            search each in the Morton codes), one thread per cell takes the nearer end: nearestGapKey, O(1).
//   pass y, z  the cells sorted by the axis-major key (nearestAxisKey; sortPairsInto carries the cell's place in the previous order), the previous keys gathered
//            into that order; a gap is a run of consecutive keys (nearestGapHead, rankHeads); one thread per gap end finds the end voxel, then one lane per
//            cell walks outwards on each side while the stop rule admits the shift (nearestScan, voxel_passes.h).  Neighbouring lanes read neighbouring
//            entries.  A pass reads the previous pass's array and writes a new one; nothing is updated in place and no lane waits on another: every loop is
//            bounded by the gap and by NEAREST_MAX_SHIFT.
//   listing  one more sort, by Morton code; the roots follow through the composed places; regions as the fill numbers them (enclosedRegionRanks); then the only
//            launch that writes the caller's arrays.
//   fill     the cells in the order of the z pass with the attribute of their nearest voxel: the edit sorts.
// No floating point.  The only atomics count and maximise the figures of mvrt_test_enclosed_nearest_stats, one per wave.
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define NB 256 // threads per workgroup, and gaps per workgroup of the x pass

namespace
{
thread_local NearestStats g_nearestStats;

enum // the slots of the device counters
{
	NS_GAPS_X = 0,
	NS_LONGEST = 1, // + axis
	NS_DEEPEST = 4,
	NS_MISSING = 5, // gap ends without a voxel: an internal error
	NS_SLOTS = 6
};

// (waveMaxInto, the maximum of a wave into a counter: voxel_passes.h)

// the vIndex of the voxel (x, y, z); a voxel that is not there is counted and gives 0
MVRT_DI uint32_t voxelIndex( const uint64_t* __restrict__ morton, uint32_t n, uint32_t x, uint32_t y, uint32_t z, unsigned long long* stats )
{
	const uint64_t i = codeIndexIn( morton, n, mortonEncode( x, y, z ) );
	if( i < n ) return (uint32_t)i;
	atomicAdd( stats + NS_MISSING, 1ull );
	return 0u;
}

// One workgroup per NB gaps, the run expansion of voxel_passes.h on the offsets of the classification.  cur = the key of pass x, keyY / place = the pair the sort
// of pass y takes, rootsX (may be null) = the root of the cell's gap
__global__ void __launch_bounds__( NB ) kNearestEmitX( const uint64_t* __restrict__ lin, const uint32_t* __restrict__ root, const uint64_t* __restrict__ offs,
														const uint64_t* __restrict__ morton, uint32_t n, uint32_t L, uint64_t* __restrict__ cur, uint64_t* __restrict__ keyY,
														uint32_t* __restrict__ place, uint32_t* __restrict__ rootsX, unsigned long long* stats )
{
	__shared__ uint32_t sOff[NB + 1];
	__shared__ uint64_t sLin[NB];
	__shared__ uint32_t sRoot[NB], sLo[NB], sHi[NB];
	const uint64_t v = (uint64_t)blockIdx.x * NB + threadIdx.x;
	const uint64_t base = stageRunOffsets<NB>( offs, n, sOff ); // (relative offsets <= NB * 2^21)
	const uint64_t a = v < n ? lin[v] : 0ull;
	const uint32_t len = v < n ? (uint32_t)( offs[v + 1] - offs[v] ) : 0u; // (offs holds n + 1 entries)
	uint32_t vLo = 0u, vHi = 0u;
	if( len ) // an enclosed gap: voxel v + 1 exists and shares the row
	{
		uint32_t x, y, z;
		nearestAxisCell( 0u, a, L, x, y, z );
		vLo = voxelIndex( morton, n, x, y, z, stats );
		vHi = voxelIndex( morton, n, x + len + 1u, y, z, stats );
	}
	sLin[threadIdx.x] = a;
	sRoot[threadIdx.x] = v < n ? root[v + 1] : 0u;
	sLo[threadIdx.x] = vLo;
	sHi[threadIdx.x] = vHi;
	const unsigned long long m = __ballot( len != 0u );
	if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 && m ) atomicAdd( stats + NS_GAPS_X, (unsigned long long)__popcll( m ) );
	waveMaxInto( stats + NS_LONGEST, len );
	__syncthreads();
	const uint32_t total = sOff[NB];
	for( uint32_t j = threadIdx.x; j < total; j += NB )
	{
		const uint32_t lo = findRun( sOff, NB, j );
		const uint32_t k = j - sOff[lo], g = sOff[lo + 1] - sOff[lo];
		uint32_t x, y, z;
		nearestAxisCell( 0u, sLin[lo], L, x, y, z );
		x += 1u + k;
		const uint64_t c = base + j;
		cur[c] = nearestGapKey( k, g, sLo[lo], sHi[lo] );
		keyY[c] = nearestAxisKey( 1u, x, y, z, L );
		place[c] = (uint32_t)c;
		if( rootsX ) rootsX[c] = sRoot[lo];
	}
}

// the previous pass's keys in the order of this pass; compOut (may be null) = the cell's place in the order of pass x
__global__ void __launch_bounds__( NB ) kNearestGather( const uint64_t* __restrict__ prev, const uint32_t* __restrict__ place, const uint32_t* __restrict__ prevComp,
														 uint32_t nCells, uint64_t* __restrict__ in, uint32_t* __restrict__ compOut )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	if( i >= nCells ) return;
	const uint32_t p = place[i];
	in[i] = prev[p];
	if( compOut ) compOut[i] = prevComp[p];
}

struct GapHead // scan input: 1 where sorted cell i starts a gap
{
	const uint64_t* keys;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return nearestGapHead( keys, i ) ? 1u : 0u; }
};

// start[g] = the first cell of gap g (start[nGaps] = nCells), ends[2 g], ends[2 g + 1] = the vIndex of the voxels before its first and behind its last cell.  An
// enclosed cell has no coordinate 0 or R - 1, so the neighbour exists in the grid; the guard keeps a broken input from wrapping
__global__ void __launch_bounds__( NB ) kNearestGapEnds( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank1, const uint64_t* __restrict__ morton, uint32_t n,
														  uint32_t L, uint32_t axis, uint32_t nCells, uint32_t nGaps, uint32_t* __restrict__ start, uint32_t* __restrict__ ends,
														  unsigned long long* stats )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	if( i >= nCells ) return;
	const bool head = nearestGapHead( keys, i ), tail = i + 1 == nCells || nearestGapHead( keys, i + 1 );
	if( i == 0 ) start[nGaps] = nCells;
	if( !head && !tail ) return;
	const uint32_t g = rank1[i] - 1u, last = ( 1u << L ) - 1u;
	uint32_t x, y, z;
	nearestAxisCell( axis, keys[i], L, x, y, z );
	const uint32_t coord = axis == 1u ? y : z;
	const bool inside = coord > 0u && coord < last;
	if( !inside ) atomicAdd( stats + NS_MISSING, 1ull );
	if( head )
	{
		start[g] = (uint32_t)i;
		ends[2u * g] = inside ? voxelIndex( morton, n, x, axis == 1u ? y - 1u : y, axis == 2u ? z - 1u : z, stats ) : 0u;
	}
	if( tail ) ends[2u * g + 1u] = inside ? voxelIndex( morton, n, x, axis == 1u ? y + 1u : y, axis == 2u ? z + 1u : z, stats ) : 0u;
}

// One lane per cell: nearestScan on its gap.  nextKeys / nextPlace (may be null): the pair the next sort takes -- nextAxis 2 = the key of pass z, 3 = the Morton
// code.  deepest: the largest d2 goes to the counters (the last pass)
__global__ void __launch_bounds__( NB ) kNearestScan( const uint64_t* __restrict__ in, const uint32_t* __restrict__ rank1, const uint32_t* __restrict__ start,
													   const uint32_t* __restrict__ ends, const uint64_t* __restrict__ keys, uint32_t axis, uint32_t L, uint32_t nCells,
													   uint64_t* __restrict__ out, uint64_t* __restrict__ nextKeys, uint32_t* __restrict__ nextPlace, uint32_t nextAxis, int deepest,
													   unsigned long long* stats )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	uint32_t gapLen = 0u, d2 = 0u;
	if( i < nCells )
	{
		const uint32_t g = rank1[i] - 1u, a = start[g], b = start[g + 1u];
		const uint64_t best = nearestScan( in + a, b - a, (uint32_t)i - a, ends[2u * g], ends[2u * g + 1u] );
		out[i] = best;
		d2 = ballKeyDist2( best );
		if( (uint32_t)i == a ) gapLen = b - a;
		if( nextKeys )
		{
			uint32_t x, y, z;
			nearestAxisCell( axis, keys[i], L, x, y, z );
			nextKeys[i] = nextAxis == 2u ? nearestAxisKey( 2u, x, y, z, L ) : mortonEncode( x, y, z );
			nextPlace[i] = (uint32_t)i;
		}
	}
	waveMaxInto( stats + NS_LONGEST + axis, gapLen );
	if( deepest ) waveMaxInto( stats + NS_DEEPEST, d2 );
}

// the root of every cell in Morton order: placeM = the cell's place in the order of pass z, comp = that place's place in the order of pass x
__global__ void __launch_bounds__( NB ) kNearestRoots( const uint32_t* __restrict__ rootsX, const uint32_t* __restrict__ comp, const uint32_t* __restrict__ placeM, uint32_t nCells,
														uint32_t* __restrict__ rootsM )
{
	const uint64_t c = (uint64_t)blockIdx.x * NB + threadIdx.x;
	if( c < nCells ) rootsM[c] = rootsX[comp[placeM[c]]];
}

// the listing, in Morton order; any output may be null.  near < nVoxels holds by construction and is checked before attrs is read
__global__ void __launch_bounds__( NB ) kNearestList( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ placeM, const uint64_t* __restrict__ val,
													   const uint32_t* __restrict__ rootsM, const uint32_t* __restrict__ firstCell, const uint32_t* __restrict__ rank1,
													   const uint2* __restrict__ attrs, uint32_t nVoxels, uint32_t nCells, uint32_t* __restrict__ xyz, uint32_t* __restrict__ region,
													   uint32_t* __restrict__ dist2, uint32_t* __restrict__ nearest, uint2* __restrict__ attribs )
{
	const uint64_t c = (uint64_t)blockIdx.x * NB + threadIdx.x;
	if( c >= nCells ) return;
	const uint64_t key = val[placeM[c]];
	const uint32_t near = ballKeyPayload( key );
	if( xyz ) mortonDecode( codes[c], xyz[c * 3], xyz[c * 3 + 1], xyz[c * 3 + 2] );
	if( region ) region[c] = rank1[firstCell[rootsM[c]]] - 1u;
	if( dist2 ) dist2[c] = ballKeyDist2( key );
	if( nearest ) nearest[c] = near;
	if( attribs ) attribs[c] = nearestAttrib( near < nVoxels ? attrs[near] : make_uint2( 0u, 0u ) );
}

// the fill: the cells in the order of the last pass
__global__ void __launch_bounds__( NB ) kNearestCells( const uint64_t* __restrict__ keys, uint32_t axis, uint32_t L, const uint64_t* __restrict__ val, const uint2* __restrict__ attrs,
														uint32_t nVoxels, uint32_t nCells, uint32_t* __restrict__ xyz, uint2* __restrict__ attribs )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	if( i >= nCells ) return;
	nearestAxisCell( axis, keys[i], L, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2] );
	const uint32_t near = ballKeyPayload( val[i] );
	attribs[i] = nearestAttrib( near < nVoxels ? attrs[near] : make_uint2( 0u, 0u ) );
}

// what the three passes leave: the keys of pass z in its order, and for the listing the pair of the Morton sort, the places in the order of pass x and the roots there
struct Passes
{
	Counters stats;
	DevBuf keysZ, val, comp, rootsX, codesA, placeA;
};
// c: the classification, with 0 < nCells < 2^32; its arrays are released on the way
int runPasses( const SurfaceSource& s, EnclosedClassified& c, bool listing, Passes& p, hipStream_t st )
{
	const uint32_t n = s.nVoxels, L = s.levels, nCells = (uint32_t)c.nCells;
	const int endBit = (int)( 3u * L );
	const dim3 cellGrid( divUp( nCells, NB ) ), block( NB );
	if( p.stats.init( NS_SLOTS, st ) ) return 1;
	unsigned long long* stats = p.stats.dev();
	DevBuf cur, keyA, placeA, keyS, place;
	if( cur.alloc( c.nCells * 8 ) || keyA.alloc( c.nCells * 8 ) || placeA.alloc( c.nCells * 4 ) || ( listing && p.rootsX.alloc( c.nCells * 4 ) ) ) return 1;
	hipLaunchKernelGGL( kNearestEmitX, dim3( divUp( n, NB ) ), block, 0, st, c.lin.as<uint64_t>(), c.root.as<uint32_t>(), c.offs.as<uint64_t>(), s.morton, n, L, cur.as<uint64_t>(),
						keyA.as<uint64_t>(), placeA.as<uint32_t>(), p.rootsX.as<uint32_t>(), stats );
	MVRT_HIP( hipGetLastError() );
	for( uint32_t axis = 1u; axis <= 2u; axis++ )
	{
		if( sortPairsInto( keyA, placeA, c.nCells, endBit, keyS, place, st ) ) return 1; // (waits)
		c.lin.release();
		c.offs.release();
		c.root.release();
		DevBuf in, comp, rank1, start, ends, out;
		const bool compose = listing && axis == 2u;
		if( in.alloc( c.nCells * 8 ) || ( compose && comp.alloc( c.nCells * 4 ) ) ) return 1;
		hipLaunchKernelGGL( kNearestGather, cellGrid, block, 0, st, cur.as<uint64_t>(), place.as<uint32_t>(), p.comp.as<uint32_t>(), nCells, in.as<uint64_t>(), comp.as<uint32_t>() );
		MVRT_HIP( hipGetLastError() );
		uint32_t nGaps = 0;
		if( rankHeadsOf( GapHead{ keyS.as<uint64_t>() }, c.nCells, rank1, &nGaps, st ) ) return 1; // (waits: the gather is done)
		cur.release();
		if( listing && axis == 1u ) p.comp = std::move( place ); // the order of pass y against the order of pass x
		else place.release();
		if( compose ) p.comp = std::move( comp );
		g_nearestStats.gaps[axis] = nGaps;
		if( start.alloc( ( (uint64_t)nGaps + 1 ) * 4 ) || ends.alloc( (uint64_t)nGaps * 8 ) || out.alloc( c.nCells * 8 ) ) return 1;
		const bool next = axis == 1u || listing;
		if( next && ( keyA.alloc( c.nCells * 8 ) || placeA.alloc( c.nCells * 4 ) ) ) return 1;
		hipLaunchKernelGGL( kNearestGapEnds, cellGrid, block, 0, st, keyS.as<uint64_t>(), rank1.as<uint32_t>(), s.morton, n, L, axis, nCells, nGaps, start.as<uint32_t>(),
							ends.as<uint32_t>(), stats );
		hipLaunchKernelGGL( kNearestScan, cellGrid, block, 0, st, in.as<uint64_t>(), rank1.as<uint32_t>(), start.as<uint32_t>(), ends.as<uint32_t>(), keyS.as<uint64_t>(), axis, L, nCells,
							out.as<uint64_t>(), next ? keyA.as<uint64_t>() : nullptr, next ? placeA.as<uint32_t>() : nullptr, axis + 1u, axis == 2u ? 1 : 0, stats );
		MVRT_HIP( hipGetLastError() );
		MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch of the pass is released here)
		cur = std::move( out );
		if( axis == 2u ) p.keysZ = std::move( keyS );
	}
	p.val = std::move( cur );
	p.codesA = std::move( keyA );
	p.placeA = std::move( placeA );
	return 0;
}
// the counters, behind the last launch; waits for the stream
int finishStats( const char* who, Passes& p, hipStream_t st )
{
	unsigned long long h[NS_SLOTS];
	if( p.stats.read( h, NS_SLOTS, st ) ) return 1;
	g_nearestStats.gaps[0] = h[NS_GAPS_X];
	for( int a = 0; a < 3; a++ ) g_nearestStats.longest[a] = h[NS_LONGEST + a];
	g_nearestStats.deepest = h[NS_DEEPEST];
	if( h[NS_MISSING] )
	{
		mvrtSetError( "%s: internal error: %llu gap ends without a voxel", who, h[NS_MISSING] );
		return 1;
	}
	return 0;
}
} // namespace

NearestStats nearestLastStats() { return g_nearestStats; }

int enclosedNearest( const SurfaceSource& s, uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, uint64_t* nCellsOut,
					 uint64_t* nRegionsOut, hipStream_t st )
{
	const char* who = "mvrt_svo_enclosed_nearest";
	g_nearestStats = NearestStats();
	EnclosedClassified c;
	if( enclosedClassify( s, &c, st ) ) return 1;
	g_nearestStats.cells = c.nCells;
	if( nCellsOut ) *nCellsOut = c.nCells;
	if( nRegionsOut ) *nRegionsOut = c.nRegions;
	if( !xyzDev && !regionDev && !dist2Dev && !nearestDev && !attribsDev ) return 0; // the sizing call: no pass is run
	if( c.nCells >= ( 1ull << 32 ) )
	{
		mvrtSetError( "%s: the %llu enclosed cells are 2^32 or more, beyond what one listing holds; nothing was written", who, (unsigned long long)c.nCells );
		return 1;
	}
	const int tail = listingTail( who, "capacity", "enclosed cells", false, capacity, c.nCells );
	if( tail != LISTING_WRITE ) return tail;
	const uint32_t nCells = (uint32_t)c.nCells;
	Passes p;
	if( runPasses( s, c, true, p, st ) ) return 1;
	DevBuf codes, placeM, rootsM, firstCell, rank1;
	if( sortPairsInto( p.codesA, p.placeA, c.nCells, (int)( 3u * s.levels ), codes, placeM, st ) ) return 1;
	if( rootsM.alloc( c.nCells * 4 ) ) return 1;
	const dim3 grid( divUp( nCells, NB ) ), block( NB );
	hipLaunchKernelGGL( kNearestRoots, grid, block, 0, st, p.rootsX.as<uint32_t>(), p.comp.as<uint32_t>(), placeM.as<uint32_t>(), nCells, rootsM.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	if( enclosedRegionRanks( rootsM.as<uint32_t>(), nCells, s.nVoxels, firstCell, rank1, st ) ) return 1;
	if( finishStats( who, p, st ) ) return 1;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	hipLaunchKernelGGL( kNearestList, grid, block, 0, st, codes.as<uint64_t>(), placeM.as<uint32_t>(), p.val.as<uint64_t>(), rootsM.as<uint32_t>(), firstCell.as<uint32_t>(),
						rank1.as<uint32_t>(), s.attrs, s.nVoxels, nCells, xyzDev, regionDev, dist2Dev, nearestDev, (uint2*)attribsDev );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int enclosedNearestUnordered( const SurfaceSource& s, DevBuf& xyz, DevBuf& attribs, uint64_t* nCells, hipStream_t st )
{
	g_nearestStats = NearestStats();
	EnclosedClassified c;
	if( enclosedClassify( s, &c, st ) ) return 1;
	g_nearestStats.cells = c.nCells;
	*nCells = c.nCells;
	if( c.nCells == 0 || (uint64_t)s.nVoxels + c.nCells >= 0xFFFFFFFFull ) return 0; // (nothing to list / the caller refuses the count)
	const uint32_t n = (uint32_t)c.nCells;
	Passes p;
	if( runPasses( s, c, false, p, st ) ) return 1;
	if( finishStats( "mvrt_svo_fill_enclosed_nearest", p, st ) ) return 1;
	if( xyz.alloc( c.nCells * 12 ) || attribs.alloc( c.nCells * 8 ) ) return 1;
	hipLaunchKernelGGL( kNearestCells, dim3( divUp( n, NB ) ), dim3( NB ), 0, st, p.keysZ.as<uint64_t>(), 2u, s.levels, p.val.as<uint64_t>(), s.attrs, s.nVoxels, n, xyz.as<uint32_t>(),
						attribs.as<uint2>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
