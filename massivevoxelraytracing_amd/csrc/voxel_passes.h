// voxel_passes.h -- the steps that the passes over a sorted voxel set share (kernels_surface.hip, kernels_fill.hip, kernels_walk.hip).
//
//   run expansion   item i of a list yields len[i] >= 0 records; offs = the n + 1 exclusive offsets of the lengths (offs[n] = the number of records).  One workgroup
//                   per B items: its records are the contiguous run [offs[first], offs[end]) of every output.  stageRunOffsets puts the group's B + 1 offsets,
//                   relative to offs[first], into LDS; thread t then takes records t, t + B, ... of the run, findRun gives the item of a record and
//                   j - sOff[item] its number within the item, so a wave writes 64 consecutive records.  Where an item's records are the set bits of a mask,
//                   nthSetBit picks the bit.
//   rows and gaps   gapLength / gapNodeOfCell on the sorted linear keys of kernels_fill.hip: the empty run between two voxels of a row, and the run an empty cell
//                   lies in.  Host-callable, so that a host program checks them against brute force (tests/hip/exterior_host.hip).
//   coarse cells    coarseHead on the shifted codes and the per-cell finish of kernels_coarsen.hip: coarseKeep, coarseAttrib (the integer means of 64-bit sums) and
//                   coarseMaxCount.  Host-callable as well (tests/hip/coarsen_host.hip).
//   elements        the neighbour tables of the two structuring elements, the presence search on the sorted codes (kernels_morph.hip) and, for the connected
//                   components (kernels_components.hip), the half of an element that sees every adjacent pair once and the search that returns the index.
//   round offsets   ballReach, ballShiftRange, ballShifted and the packed key ( d2 << 32 | payload ) of kernels_ball.hip: the shifts an entry of a distance pass sends
//                   records to, clipped to the grid and to the radius.  Host-callable (tests/hip/ball_host.hip).
//   nearest voxel   nearestAxisKey / nearestAxisCell / nearestGapHead (the cells of a line as consecutive keys), nearestGapKey, nearestEndKey, nearestGoOn and
//                   nearestScan of kernels_nearest.hip: the minimum of the packed key over a gap of enclosed cells and its two end voxels.  Host-callable
//                   (tests/hip/nearest_host.hip).
//   nearest query   nearestBoxDist2, nearestChildRange, nearestChildOrder, nearestSeed, nearestPairBelow and the whole walk nearestQueryWalk of kernels_query.hip: the
//                   nearest voxel of an arbitrary lattice point by branch and bound on the sorted codes.  Host-callable (tests/hip/query_host.hip).
//   two sets        combineTranslate (a code moved by an integer offset and clipped to a grid) of kernels_combine.hip, and combineWindow / codeIndexInRange: the
//                   partner search of a group of ascending codes, bounded once per group.  Host-callable (tests/hip/combine_host.hip).
//   resampling      resamplePoint (the point rule of mvrt_cell_transform), resampleBox / resampleBoxShift / resampleBoxHoldsVoxel (the conservative test of a node
//                   of the destination grid) and resampleTransformOk of kernels_resample.hip.  Host-callable (tests/hip/resample_host.hip).
//   union-find      ufLoad / ufStore / ufFind / ufUnite / ufRoot: the lock-free union-find over node ids that kernels_fill.hip runs on the gaps and
//                   kernels_components.hip on the voxels.  Device only.
//   wave sums       waveSum / waveMax / waveMin over the 64 lanes, templates on the type the shuffles move, and waveAddInto / waveMaxInto, which end in one atomic
//                   of lane 0 into a 64-bit counter: the counts of kernels_surface.hip, kernels_fill.hip, kernels_nearest.hip and kernels_query.hip.  Device only.
//   host steps      exclusiveOffsets (the offsets above), sortPairsInto (a radix sort out of place that gives the input back) and rankHeads (head flags of sorted
//                   entries -> rank + 1 of every entry and the number of runs).  Each allocates its output itself, runs hipcub through withCubTemp and has waited
//                   for the stream when it returns.  exclusiveOffsetsOf / rankHeadsOf take the scan's input as a functor of the item's number and build the
//                   counting and transform iterators themselves: the scans over a functor of eleven kernels_*.hip go through them (the three scans of kernels_surface.hip
//                   over a byte array keep their transform iterator over the pointer, the per-level scan of kernels_resample.hip its hand-built pair).  KeyHead is the one head functor "sorted key differs from
//                   its predecessor" (kernels_morph.hip, kernels_ball.hip, kernels_surface.hip).  Counters is the block of 64-bit counters of one call: allocated
//                   and zeroed on the stream, read back with a wait (kernels_surface.hip, kernels_fill.hip, kernels_nearest.hip, kernels_query.hip).
//   list steps      not here: the steps on whole sorted voxel lists that the operators share (merge, gather of attributes, emission scan, compaction by a mask, the
//                   driver of a dilate / erode / close / open, the tail of a listing) are declared in launch.h under "sorted voxel lists" and live in kernels_list.hip.
#pragma once
#include <hipcub/hipcub.hpp>

#include "devbuf.h"

// ---- run expansion ----------------------------------------------------------------------------------------------------------------------------------------
// Called by all B threads of the group, before the __syncthreads() that also covers what the kernel stages for itself.  sOff[t] = offs[first + t] - offs[first]
// for t = 0 .. B; the last group reads offs[n] for every item past the end, so its tail repeats the total.  Returns offs[first], the group's place in the output.
template <uint32_t B> MVRT_DI uint64_t stageRunOffsets( const uint64_t* __restrict__ offs, uint64_t n, uint32_t* sOff )
{
	const uint64_t first = (uint64_t)blockIdx.x * B;
	const uint64_t v = first + threadIdx.x;
	const uint64_t base = offs[first];
	sOff[threadIdx.x] = (uint32_t)( offs[v < n ? v : n] - base );
	if( threadIdx.x == 0 ) sOff[B] = (uint32_t)( offs[first + B < n ? first + B : n] - base );
	return base;
}
// the last i < count with sOff[i] <= j, for sOff ascending from sOff[0] = 0: an item of length 0 repeats the offset of the next one and is passed over
MVRT_HDI uint32_t findRun( const uint32_t* sOff, uint32_t count, uint32_t j )
{
	uint32_t lo = 0, hi = count;
	while( hi - lo > 1 )
	{
		const uint32_t mid = ( lo + hi ) >> 1;
		if( sOff[mid] <= j ) lo = mid;
		else hi = mid;
	}
	return lo;
}
// the position of the r-th set bit of mask, r counted from 0 at the lowest (~0 where the mask has r bits or fewer)
MVRT_HDI uint32_t nthSetBit( uint32_t mask, uint32_t r )
{
	for( ; r > 0; r-- ) mask &= mask - 1u;
	return mask == 0u ? ~0u : (uint32_t)__builtin_ctz( mask );
}

// ---- rows and gaps (kernels_fill.hip) -----------------------------------------------------------------------------------------------------------------------
// lin: the n sorted linear keys ( z << 2L | y << L | x ) of the voxels.  Gap i exists when voxels i and i + 1 share a row and are not adjacent; its cells are
// x in [ x(i) + 1, x(i + 1) - 1 ]
MVRT_HDI uint64_t gapLength( const uint64_t* __restrict__ lin, uint32_t n, uint32_t L, uint64_t i )
{
	if( i + 1 >= n ) return 0;
	const uint64_t a = lin[i], b = lin[i + 1];
	return ( a >> L ) == ( b >> L ) ? b - a - 1ull : 0ull;
}
// The union-find node of the empty in-grid cell with the linear key `key` (not in lin): node j = gap j - 1 when the voxels j - 1 and j of the list stand left and
// right of the cell in its row; 0 = EXTERIOR when the cell lies in the run before the first voxel of its row, in the run behind the last one or in a row
// without voxels, which hold a border cell and are exterior by themselves.  One bounded search; reads lin[j - 1] and lin[j] only for 0 < j < n.
MVRT_HDI uint32_t gapNodeOfCell( const uint64_t* __restrict__ lin, uint32_t n, uint32_t L, uint64_t key )
{
	const uint64_t j = lowerBound( lin, 0, n, key );
	if( j == 0 || j >= n ) return 0u;
	const uint64_t row = key >> L;
	return ( lin[j - 1] >> L ) == row && ( lin[j] >> L ) == row ? (uint32_t)j : 0u;
}

// ---- coarse cells (kernels_coarsen.hip) -----------------------------------------------------------------------------------------------------------------------
// codes: the n sorted voxel codes, shift = 3 * levelsDown <= 60.  The coarse cell of a voxel is code >> shift, still ascending: a cell is one run of entries, and
// entry i starts one when it is the first of the list or its cell differs from its predecessor's.  Host-callable like the gap helpers (tests/hip/coarsen_host.hip).
MVRT_HDI bool coarseHead( const uint64_t* __restrict__ codes, uint64_t i, uint32_t shift ) { return i == 0 || ( codes[i] >> shift ) != ( codes[i - 1] >> shift ); }
// the fine voxels a coarse cell can hold, 8^levelsDown: the largest legal minCount (levelsDown <= 20: up to 2^60)
MVRT_HDI uint64_t coarseMaxCount( uint32_t levelsDown ) { return 1ull << ( 3u * levelsDown ); }
MVRT_HDI bool coarseKeep( uint64_t count, uint64_t minCount ) { return count >= minCount; }
// floor( sum / count ) for count >= 1 and sum <= 255 * count; the 32-bit division where both fit (nearly every cell), the quotient is the same
MVRT_HDI uint32_t coarseMean( uint64_t sum, uint64_t count )
{
	return ( ( sum | count ) >> 32 ) == 0 ? (uint32_t)sum / (uint32_t)count : (uint32_t)( sum / count );
}
// the attribute of a cell from the exact sums of R, G, B of colour (sums[0..2]) and of emission (sums[3..5]) over its count voxels: the reference's unique rule
// (voxKernel.cu:201-210) with sums that cannot overflow; both alpha bytes are 255
MVRT_HDI uint2 coarseAttrib( const uint64_t sums[6], uint64_t count )
{
	uint2 a;
	a.x = coarseMean( sums[0], count ) | coarseMean( sums[1], count ) << 8 | coarseMean( sums[2], count ) << 16 | 255u << 24;
	a.y = coarseMean( sums[3], count ) | coarseMean( sums[4], count ) << 8 | coarseMean( sums[5], count ) << 16 | 255u << 24;
	return a;
}

// ---- structuring elements (kernels_morph.hip) ---------------------------------------------------------------------------------------------------------------
// element 0 = the 6 face neighbours, 1 = the 26 neighbours of the 3x3x3 block (MVRT_MORPH_FACES / MVRT_MORPH_CUBE, mvrt.h).  Neighbour j of a cell, j in
// [0, morphNeighbours( element )): faces in the order -x, +x, -y, +y, -z, +z; the block in the order of t = ( dz + 1 ) * 9 + ( dy + 1 ) * 3 + ( dx + 1 ) with the
// centre t = 13 left out.  Host-callable like the gap and coarse helpers (tests/hip/morph_host.hip).
MVRT_HDI bool morphElementOk( int element ) { return element == 0 || element == 1; }
MVRT_HDI uint32_t morphNeighbours( int element ) { return element == 0 ? 6u : 26u; }
MVRT_HDI void morphOffset( int element, uint32_t j, int& dx, int& dy, int& dz )
{
	if( element == 0 )
	{
		const int s = ( j & 1u ) ? 1 : -1;
		dx = j < 2u ? s : 0;
		dy = j >= 2u && j < 4u ? s : 0;
		dz = j >= 4u ? s : 0;
		return;
	}
	const uint32_t t = j < 13u ? j : j + 1u;
	dx = (int)( t % 3u ) - 1;
	dy = (int)( ( t / 3u ) % 3u ) - 1;
	dz = (int)( t / 9u ) - 1;
}
// neighbour j of the cell (x, y, z) of a grid of R = 2^levels <= 2^21 cells per axis: false when it lies outside the grid (a coordinate of -1 wraps to 2^32 - 1,
// one of R is R: neither is below R, so nothing is ever folded back into the 21 bits per axis of a code), else true and *code = its Morton code
MVRT_HDI bool morphNeighbour( uint32_t x, uint32_t y, uint32_t z, uint32_t levels, int element, uint32_t j, uint64_t* code )
{
	int dx, dy, dz;
	morphOffset( element, j, dx, dy, dz );
	const uint32_t R = 1u << levels, nx = x + (uint32_t)dx, ny = y + (uint32_t)dy, nz = z + (uint32_t)dz;
	if( nx >= R || ny >= R || nz >= R ) return false;
	*code = mortonEncode( nx, ny, nz );
	return true;
}
MVRT_HDI bool codePresentIn( const uint64_t* __restrict__ codes, uint64_t n, uint64_t code )
{
	const uint64_t i = lowerBound( codes, 0, n, code );
	return i < n && codes[i] == code;
}
// the index of `code` among the n sorted unique codes, n where it is not one of them: codePresentIn that says where
MVRT_HDI uint64_t codeIndexIn( const uint64_t* __restrict__ codes, uint64_t n, uint64_t code )
{
	const uint64_t i = lowerBound( codes, 0, n, code );
	return i < n && codes[i] == code ? i : n;
}
// The half of an element (kernels_components.hip): neighbour j belongs to it when its offset (dz, dy, dx) is lexicographically below (0, 0, 0) -- the faces -x, -y,
// -z (even j), the first 13 of the block (t < 13).  The other half holds the negated offsets, so of an adjacent pair {a, b} exactly one of a -> b and b -> a
// lies in the half: a pass over the halves of all voxels sees every unordered pair once.  3 of 6, 13 of 26 (tests/hip/components_host.hip)
MVRT_HDI bool componentHalf( int element, uint32_t j ) { return element == 0 ? ( j & 1u ) == 0u && j < 6u : j < 13u; }
// bit j = neighbour j of voxel (x, y, z) lies inside the grid and is not among the n sorted codes: the cells a dilation step adds next to this voxel, and the
// reason an erosion step removes it (any bit set; outside the grid counts as occupied)
MVRT_HDI uint32_t morphEmptyMask( const uint64_t* __restrict__ codes, uint64_t n, uint32_t levels, int element, uint64_t code )
{
	uint32_t x, y, z, mask = 0u;
	mortonDecode( code, x, y, z );
	const uint32_t nb = morphNeighbours( element );
	for( uint32_t j = 0; j < nb; j++ )
	{
		uint64_t c;
		if( morphNeighbour( x, y, z, levels, element, j, &c ) && !codePresentIn( codes, n, c ) ) mask |= 1u << j;
	}
	return mask;
}

// ---- round offsets (kernels_ball.hip) -----------------------------------------------------------------------------------------------------------------------
// The exact squared distance is a sum over the axes, so the band of cells within rho of a seed list is made by three passes, one per axis: an
// entry ( code, d2 << 32 | payload ) yields the in-grid cells at shift s on the axis of the pass with d2 + s * s <= rho.  Host-callable like the morph helpers
// (tests/hip/ball_host.hip).
// floor( sqrt( rho ) ) for rho < 4096 without floating point: the reach of a ball, 32 at most for a legal radius
MVRT_HDI uint32_t ballReach( uint32_t rho )
{
	uint32_t k = 0u;
	for( uint32_t bit = 32u; bit != 0u; bit >>= 1 )
		if( ( k + bit ) * ( k + bit ) <= rho ) k += bit;
	return k;
}
MVRT_HDI uint64_t ballKey( uint32_t d2, uint32_t payload ) { return (uint64_t)d2 << 32 | payload; }
MVRT_HDI uint32_t ballKeyDist2( uint64_t key ) { return (uint32_t)( key >> 32 ); }
MVRT_HDI uint32_t ballKeyPayload( uint64_t key ) { return (uint32_t)key; }
MVRT_HDI uint32_t ballAxisCoord( uint64_t code, uint32_t axis ) { return compactBy3( code >> axis ); }
// The shifts an entry at coordinate `coord` of the pass's axis, with squared distance d2 <= rho so far, sends records to: *first, *first + 1, ..., *first + count - 1
// with count the return value, at least 1 (the shift 0).  m = ballReach( rho - d2 ) bounds |s|; below, the shift stops at coordinate 0, above at R - 1: a
// coordinate of -1 or R does not exist, R = 2^21 included, so nothing is ever folded back into the 21 bits per axis of a code.
MVRT_HDI uint32_t ballShiftRange( uint32_t coord, uint32_t levels, uint32_t d2, uint32_t rho, int32_t* first )
{
	const uint32_t m = ballReach( rho - d2 ), above = ( 1u << levels ) - 1u - coord;
	const uint32_t down = m < coord ? m : coord, up = m < above ? m : above;
	*first = -(int32_t)down;
	return down + up + 1u;
}
// the cell `code` names moved by s cells along the axis (0 = x, 1 = y, 2 = z) of a grid of R = 2^levels <= 2^21 cells per axis: false when it leaves the grid,
// else true and *codeOut = its code.  The sum is taken in 64 bits like combineTranslate's
MVRT_HDI bool ballShifted( uint64_t code, uint32_t levels, uint32_t axis, int32_t s, uint64_t* codeOut )
{
	const int64_t c = (int64_t)ballAxisCoord( code, axis ) + s;
	if( c < 0 || c >= (int64_t)1 << levels ) return false;
	*codeOut = ( code & ~( 0x1249249249249249ull << axis ) ) | splitBy3( (uint32_t)c ) << axis;
	return true;
}
// the key of the record at shift s: the distance field grows by s * s, the payload stays.  Adding the same constant to both keeps the order of two keys
MVRT_HDI uint64_t ballShiftKey( uint64_t key, int32_t s ) { return key + ( (uint64_t)( (uint32_t)( s * s ) ) << 32 ); }

// ---- nearest voxel of the enclosed cells (kernels_nearest.hip) ------------------------------------------------------------------------------------------------
// Three passes over the gaps, one per axis: along an axis the enclosed cells of a line fall into gaps, maximal runs of cells with a voxel at
// either end, and a cell's packed key ( d2 << 32 | vIndex ) is minimised over its own gap and the gap's two end voxels.  d2 of an enclosed cell is below 2^20
// (mvrt.h), so a shift beyond NEAREST_MAX_SHIFT never wins: the scan does not go further, and the x pass stores the square of NEAREST_MAX_SHIFT + 1 for a voxel
// further off.  Such an entry loses against the true minimum wherever it is read, and the sum of three such squares fits the distance field.  Host-callable
// (tests/hip/nearest_host.hip runs the passes with exactly these functions).
#define NEAREST_MAX_SHIFT 1023u
// The key of a line of cells along `axis` (0 = x, 1 = y, 2 = z): the coordinate of that axis in the low L bits, so that the cells of one line are consecutive
// keys.  An enclosed cell has no coordinate 0 or R - 1: key + 1 never carries into another line, and two sorted keys that differ by 1 are face neighbours
MVRT_HDI uint64_t nearestAxisKey( uint32_t axis, uint32_t x, uint32_t y, uint32_t z, uint32_t L )
{
	const uint64_t a = axis == 0u ? x : axis == 1u ? y : z, b = axis == 0u ? y : x, c = axis == 2u ? y : z;
	return ( (uint64_t)c << ( 2u * L ) ) | ( (uint64_t)b << L ) | a;
}
MVRT_HDI void nearestAxisCell( uint32_t axis, uint64_t key, uint32_t L, uint32_t& x, uint32_t& y, uint32_t& z )
{
	const uint64_t m = ( 1ull << L ) - 1ull;
	const uint32_t a = (uint32_t)( key & m ), b = (uint32_t)( ( key >> L ) & m ), c = (uint32_t)( key >> ( 2u * L ) );
	x = axis == 0u ? a : b;
	y = axis == 0u ? b : axis == 1u ? a : c;
	z = axis == 2u ? a : c;
}
MVRT_HDI bool nearestGapHead( const uint64_t* __restrict__ keys, uint64_t i ) { return i == 0 || keys[i] != keys[i - 1] + 1ull; }
// the candidate of the voxel at shift s >= 1 with index vIndex; s is clamped as said above
MVRT_HDI uint64_t nearestEndKey( uint64_t s, uint32_t vIndex )
{
	const uint32_t c = s > NEAREST_MAX_SHIFT ? NEAREST_MAX_SHIFT + 1u : (uint32_t)s;
	return ballKey( c * c, vIndex );
}
// pass x: cell k of a gap of g cells between the voxels vLo (left of cell 0) and vHi (right of cell g - 1)
MVRT_HDI uint64_t nearestGapKey( uint64_t k, uint64_t g, uint32_t vLo, uint32_t vHi )
{
	const uint64_t lo = nearestEndKey( k + 1ull, vLo ), hi = nearestEndKey( g - k, vHi );
	return lo < hi ? lo : hi;
}
// The stop rule: a candidate at shift s has a distance of at least s * s, so a side is left once s * s > the best d2 -- not >=: a tie at equal d2 can still lower
// the vIndex
MVRT_HDI bool nearestGoOn( uint32_t s, uint64_t best ) { return s <= NEAREST_MAX_SHIFT && s * s <= ballKeyDist2( best ); }
// passes y and z: seg = the keys the previous pass left for the g cells of one gap, in the order of the axis; the result for cell k.  Reads seg[k] and, per
// side, the cells at the shifts the stop rule admits; where a side reaches the end of the gap under that rule, the end voxel is the last candidate
MVRT_HDI uint64_t nearestScan( const uint64_t* __restrict__ seg, uint32_t g, uint32_t k, uint32_t vLo, uint32_t vHi )
{
	uint64_t best = seg[k];
	for( uint32_t s = 1u; nearestGoOn( s, best ); s++ )
	{
		const uint64_t c = s <= k ? ballShiftKey( seg[k - s], (int32_t)s ) : nearestEndKey( s, vLo );
		best = c < best ? c : best;
		if( s > k ) break;
	}
	const uint32_t above = g - 1u - k; // cells behind k
	for( uint32_t s = 1u; nearestGoOn( s, best ); s++ )
	{
		const uint64_t c = s <= above ? ballShiftKey( seg[k + s], (int32_t)s ) : nearestEndKey( s, vHi );
		best = c < best ? c : best;
		if( s > above ) break;
	}
	return best;
}
// the 8 bytes a cell takes from its nearest voxel: colour RGB and emission RGB, both alpha bytes 255 (the rule of MVRT_VOXEL_SET)
MVRT_HDI uint2 nearestAttrib( uint2 a )
{
	a.x |= 0xFF000000u;
	a.y |= 0xFF000000u;
	return a;
}

// ---- nearest voxel of arbitrary lattice points (kernels_query.hip) ----------------------------------------------------------------------------------------------
// An exact branch-and-bound descent on the n sorted codes.  A node is a code prefix at a depth d in [0, L] with its range [lo, hi) of the code
// array: depth 0 is the grid with [0, n), depth L a voxel, whose place in the array is its vIndex.  A query q is three int32, each in [-2^22, 2^22]; a
// coordinate difference is below 2^23 in magnitude, a square below 2^46 and a sum of three below 2^48: everything is taken in int64 / uint64 and nothing can
// wrap (d2 itself stays below 2^47).  Host-callable (tests/hip/query_host.hip runs the whole walk against brute force).
#define NEAREST_QUERY_NONE_D2 0xFFFFFFFFFFFFFFFFull // no voxel within the limit: dist2 = UINT64_MAX, nearest = 0xFFFFFFFF, attribs 0
#define NEAREST_QUERY_NONE 0xFFFFFFFFu
#define NEAREST_QUERY_COORD_MAX ( 1 << 22 )
#define NEAREST_QUERY_RUN 8u // a child of at most this many voxels is compared voxel by voxel: cheaper than three more levels of searches
// the squared distance from q to the cells [c, c + 2^s - 1] per axis: 0 inside, else to the nearest face, edge or corner cell
MVRT_HDI uint64_t nearestBoxDist2( int32_t qx, int32_t qy, int32_t qz, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t s )
{
	const int64_t span = ( (int64_t)1 << s ) - 1;
	const int64_t q[3] = { qx, qy, qz }, c[3] = { (int64_t)cx, (int64_t)cy, (int64_t)cz };
	uint64_t d2 = 0;
	for( int k = 0; k < 3; k++ )
	{
		const int64_t d = q[k] < c[k] ? c[k] - q[k] : q[k] > c[k] + span ? q[k] - c[k] - span : 0;
		d2 += (uint64_t)d * (uint64_t)d;
	}
	return d2;
}
MVRT_HDI uint64_t nearestPointDist2( int32_t qx, int32_t qy, int32_t qz, uint64_t code )
{
	uint32_t x, y, z;
	mortonDecode( code, x, y, z );
	return nearestBoxDist2( qx, qy, qz, x, y, z, 0u );
}
// ( d2, vIndex ) compared as a pair: the candidate replaces the best when it is nearer, or as near with a lower index
MVRT_HDI bool nearestPairBelow( uint64_t d2, uint32_t v, uint64_t bestD2, uint32_t bestV ) { return d2 < bestD2 || ( d2 == bestD2 && v < bestV ); }
// The pruning rule, which is the correctness of the walk: a box is skipped only when its distance EXCEEDS the best d2 so far or the limit -- not >=: a voxel
// at exactly the best d2 can still lower the vIndex (the stop rule of nearestGoOn)
MVRT_HDI bool nearestBoxSkipped( uint64_t boxD2, uint64_t bestD2, uint64_t maxDist2 ) { return boxD2 > bestD2 || boxD2 > maxDist2; }
// the k-th child to visit, k in [0, 8), for a query in octant `oct` of the node (bit a = q is at or beyond the node's centre on axis a): the octant itself, its
// three face neighbours, its three edge neighbours, the opposite one.  The order only decides how soon the bound tightens, never the answer
MVRT_HDI uint32_t nearestChildOrder( uint32_t oct, uint32_t k ) { return oct ^ ( ( 0x76534210u >> ( 4u * k ) ) & 7u ); }
MVRT_HDI uint32_t nearestOctant( int32_t qx, int32_t qy, int32_t qz, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t s ) // s = log2 of the CHILD size
{
	const int64_t h = (int64_t)1 << s;
	return ( qx >= (int64_t)cx + h ? 1u : 0u ) | ( qy >= (int64_t)cy + h ? 2u : 0u ) | ( qz >= (int64_t)cz + h ? 4u : 0u );
}
// the range of child c (its size 2^s per axis) of the node with code prefix `prefix` (the code of its lowest cell) inside the node's range [lo, hi): two
// searches in the range, none where the child is the first or the last of its node.  ( prefix + ( c + 1 ) << 3s ) <= 2^63
MVRT_HDI void nearestChildRange( const uint64_t* __restrict__ codes, uint64_t lo, uint64_t hi, uint64_t prefix, uint32_t c, uint32_t s, uint64_t* cLo, uint64_t* cHi )
{
	const uint64_t first = prefix | (uint64_t)c << ( 3u * s );
	*cLo = c == 0u ? lo : lowerBound( codes, lo, hi, first );
	*cHi = c == 7u ? hi : lowerBound( codes, *cLo, hi, first + ( 1ull << ( 3u * s ) ) );
}
// the bound before the descent, from real voxels: the one or two codes next to where the code of q, clamped into the grid, would stand.  Every candidate is the
// true distance to a real voxel, so nothing can fall below the minimum
MVRT_HDI uint32_t nearestSeed( const uint64_t* __restrict__ codes, uint64_t n, uint32_t L, int32_t qx, int32_t qy, int32_t qz, uint64_t* bestD2, uint32_t* bestV )
{
	uint32_t taken = 0u;
	const int32_t last = (int32_t)( ( 1u << L ) - 1u );
	const uint32_t x = (uint32_t)( qx < 0 ? 0 : qx > last ? last : qx ), y = (uint32_t)( qy < 0 ? 0 : qy > last ? last : qy ), z = (uint32_t)( qz < 0 ? 0 : qz > last ? last : qz );
	const uint64_t j = lowerBound( codes, 0, n, mortonEncode( x, y, z ) );
	for( uint64_t i = j > 0 ? j - 1 : 0; i < n && i <= j; i++ )
	{
		const uint64_t d2 = nearestPointDist2( qx, qy, qz, codes[i] );
		if( nearestPairBelow( d2, (uint32_t)i, *bestD2, *bestV ) ) *bestD2 = d2, *bestV = (uint32_t)i;
		taken++;
	}
	return taken; // the voxels compared
}
// The backtracking state of one walk: per depth d in [0, L) the range of the node there, kept by the caller (the kernel: LDS, one column per lane; a host
// program: an array), and the number of children already tried, 4 bits per depth in two words that stay in registers
struct NearestQueryHostStack
{
	uint32_t lo[21], hi[21];
	MVRT_HDI void put( uint32_t d, uint32_t l, uint32_t h ) { lo[d] = l, hi[d] = h; }
	MVRT_HDI void get( uint32_t d, uint32_t& l, uint32_t& h ) const { l = lo[d], h = hi[d]; }
};
MVRT_HDI uint32_t nearestTriedGet( uint64_t w0, uint64_t w1, uint32_t d ) { return (uint32_t)( ( d < 16u ? w0 >> ( 4u * d ) : w1 >> ( 4u * ( d - 16u ) ) ) & 15ull ); }
MVRT_HDI void nearestTriedSet( uint64_t& w0, uint64_t& w1, uint32_t d, uint32_t k )
{
	if( d < 16u ) w0 = ( w0 & ~( 15ull << ( 4u * d ) ) ) | (uint64_t)k << ( 4u * d );
	else w1 = ( w1 & ~( 15ull << ( 4u * ( d - 16u ) ) ) ) | (uint64_t)k << ( 4u * ( d - 16u ) );
}
struct NearestQueryAnswer
{
	uint64_t d2;	  // NEAREST_QUERY_NONE_D2: no voxel within maxDist2
	uint32_t near;	  // the lowest vIndex among the voxels at d2
	uint32_t visits;  // non-empty children whose box was tested
	uint32_t compared; // voxels whose distance was taken, the seed's included
};
// The whole query: n >= 1 sorted unique codes of a grid of L in [1, 21] levels, q within +-NEAREST_QUERY_COORD_MAX, n < 2^32.  Every loop is bounded: a
// (node, child) pair is taken once, a node has 8 children and a path L nodes; a run by NEAREST_QUERY_RUN.  seed == 0 starts without a bound (measuring only)
template <class Stack>
MVRT_HDI NearestQueryAnswer nearestQueryWalk( const uint64_t* __restrict__ codes, uint64_t n, uint32_t L, int32_t qx, int32_t qy, int32_t qz, uint64_t maxDist2, int seed, Stack& stack )
{
	NearestQueryAnswer r = { NEAREST_QUERY_NONE_D2, NEAREST_QUERY_NONE, 0u, 0u };
	if( seed ) r.compared = nearestSeed( codes, n, L, qx, qy, qz, &r.d2, &r.near );
	if( r.d2 == 0ull ) return r; // the query is a voxel: the voxels are distinct, nothing else is as near, and 0 is within every limit
	uint64_t tried0 = 0, tried1 = 0, prefix = 0;
	uint32_t d = 0, lo = 0, hi = (uint32_t)n, cx = 0, cy = 0, cz = 0, k = 0;
	for( ;; )
	{
		if( k == 8u ) // this node is done: back to its parent
		{
			if( d == 0u ) break;
			d--;
			stack.get( d, lo, hi );
			k = nearestTriedGet( tried0, tried1, d );
			const uint32_t keep = ~( ( 1u << ( L - d ) ) - 1u ); // (L - d <= 21)
			cx &= keep, cy &= keep, cz &= keep;
			prefix &= ~( ( 1ull << ( 3u * ( L - d ) ) ) - 1ull );
			continue;
		}
		const uint32_t s = L - d - 1u; // log2 of the child size
		const uint32_t c = nearestChildOrder( nearestOctant( qx, qy, qz, cx, cy, cz, s ), k++ );
		uint64_t cLo, cHi;
		nearestChildRange( codes, lo, hi, prefix, c, s, &cLo, &cHi );
		if( cLo == cHi ) continue; // no voxel below this child
		const uint32_t kx = cx | ( c & 1u ) << s, ky = cy | ( ( c >> 1 ) & 1u ) << s, kz = cz | ( c >> 2 ) << s;
		r.visits++;
		if( nearestBoxSkipped( nearestBoxDist2( qx, qy, qz, kx, ky, kz, s ), r.d2, maxDist2 ) ) continue;
		if( s == 0u || cHi - cLo <= NEAREST_QUERY_RUN ) // a voxel, or a short run of them
		{
			for( uint64_t i = cLo; i < cHi; i++ )
			{
				const uint64_t d2 = nearestPointDist2( qx, qy, qz, codes[i] );
				if( nearestPairBelow( d2, (uint32_t)i, r.d2, r.near ) ) r.d2 = d2, r.near = (uint32_t)i;
			}
			r.compared += (uint32_t)( cHi - cLo );
			continue;
		}
		stack.put( d, lo, hi );
		nearestTriedSet( tried0, tried1, d, k );
		d++;
		lo = (uint32_t)cLo, hi = (uint32_t)cHi;
		cx = kx, cy = ky, cz = kz;
		prefix |= (uint64_t)c << ( 3u * s );
		k = 0u;
	}
	if( r.d2 > maxDist2 ) r.d2 = NEAREST_QUERY_NONE_D2, r.near = NEAREST_QUERY_NONE; // (a seed beyond the limit, or nothing in reach)
	return r;
}
// the query of voxel `code` of another set moved by -o into this one's cell space: q = v - o, |q| <= 2^21 + 2^21
MVRT_HDI void nearestQueryOfVoxel( uint64_t code, const int32_t o[3], int32_t* qx, int32_t* qy, int32_t* qz )
{
	uint32_t x, y, z;
	mortonDecode( code, x, y, z );
	*qx = (int32_t)x - o[0], *qy = (int32_t)y - o[1], *qz = (int32_t)z - o[2];
}
// the 8 bytes a voxel with the attribute `own` ends with when it takes the words `flags` names (1 = colour, 2 = emission) from `from`, as MVRT_VOXEL_SET stores them
MVRT_HDI uint2 nearestTransferAttrib( uint2 own, uint2 from, uint32_t flags )
{
	return nearestAttrib( make_uint2( ( flags & 1u ) ? from.x : own.x, ( flags & 2u ) ? from.y : own.y ) );
}

// ---- two sets (kernels_combine.hip) -------------------------------------------------------------------------------------------------------------------------
// The cell `code` names, moved by the offset o (each component in [-2^21, 2^21]) inside a grid of R = 2^levels <= 2^21 cells per axis: false when it leaves the
// grid, else true and *codeOut = its code there.  The sums are taken in 64 bits, where 2^21 - 1 + 2^21 and 0 - 2^21 are ordinary numbers: a coordinate of -1 or R is
// outside, nothing is folded back into the 21 bits per axis of a code.  The source grid may be larger or smaller than R.  Host-callable (tests/hip/combine_host.hip)
MVRT_HDI bool combineTranslate( uint64_t code, const int32_t o[3], uint32_t levels, uint64_t* codeOut )
{
	uint32_t x, y, z;
	mortonDecode( code, x, y, z );
	const int64_t R = (int64_t)1 << levels, nx = (int64_t)x + o[0], ny = (int64_t)y + o[1], nz = (int64_t)z + o[2];
	if( nx < 0 || nx >= R || ny < 0 || ny >= R || nz < 0 || nz >= R ) return false;
	*codeOut = mortonEncode( (uint32_t)nx, (uint32_t)ny, (uint32_t)nz );
	return true;
}
// (kCombineClassify searches the whole list per lane: with one thread finding the window for its workgroup the kernel was measured a third slower, DESIGN.md 5.20.  The
// two helpers below are that bounded search, host-callable and checked against codeIndexIn by tests/hip/combine_host.hip.)
// The window of the n sorted unique codes that a group of ascending codes first <= ... <= last needs: every entry below *lo is below `first`, every entry from *hi
// on is not below `last`, so for each code c of the group lowerBound( codes, *lo, *hi, c ) == lowerBound( codes, 0, n, c ).  0 <= *lo <= *hi <= n; n == 0 gives 0, 0
MVRT_HDI void combineWindow( const uint64_t* __restrict__ codes, uint64_t n, uint64_t first, uint64_t last, uint64_t* lo, uint64_t* hi )
{
	*lo = lowerBound( codes, 0, n, first );
	*hi = lowerBound( codes, *lo, n, last );
}
// codeIndexIn for a code of the group, searched in its window alone: the index of `code` among the n codes, n where it is not one of them
MVRT_HDI uint64_t codeIndexInRange( const uint64_t* __restrict__ codes, uint64_t n, uint64_t lo, uint64_t hi, uint64_t code )
{
	const uint64_t i = lowerBound( codes, lo, hi, code );
	return i < n && codes[i] == code ? i : n;
}

// ---- affine resampling (kernels_resample.hip) ---------------------------------------------------------------------------------------------------------------
// The inverse map of mvrt_cell_transform (mvrt.h): m in Q24 with |m[k]| <= 2^30, t in Q25 with |t[i]| <= 2^52.  A sample coordinate 2 * c + 1 is below 2^22, so a
// product is below 2^52 in magnitude and a sum of three plus t below 2^55: nothing here can wrap.  Host-callable (tests/hip/resample_host.hip, which runs under
// UBSan's signed-overflow check and compares with __int128).
#define RESAMPLE_FRAC_BITS 24
struct ResampleXf
{
	int64_t m[9], t[3];
};
MVRT_HDI bool resampleTransformOk( const int64_t m[9], const int64_t t[3] )
{
	const int64_t mMax = (int64_t)1 << 30, tMax = (int64_t)1 << 52;
	for( int k = 0; k < 9; k++ )
		if( m[k] < -mMax || m[k] > mMax ) return false;
	for( int i = 0; i < 3; i++ )
		if( t[i] < -tMax || t[i] > tMax ) return false;
	return true;
}
// floor( p / 2^(F + 1) ) towards minus infinity, written without a shift of a negative number
MVRT_HDI int64_t resampleFloor( int64_t p )
{
	const int64_t one = (int64_t)1 << ( RESAMPLE_FRAC_BITS + 1 );
	return p >= 0 ? p / one : -( ( -p + one - 1 ) / one );
}
// The point rule: the source cell s the centre of the destination cell c = (c0, c1, c2), each below 2^21, maps into.  True when s lies in [0, 2^srcLevels)^3;
// s is written either way, a coordinate outside the grid as it is (it fits: |s| < 2^30)
MVRT_HDI bool resamplePoint( const ResampleXf& xf, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t srcLevels, int64_t s[3] )
{
	const int64_t q0 = 2 * (int64_t)c0 + 1, q1 = 2 * (int64_t)c1 + 1, q2 = 2 * (int64_t)c2 + 1, Rs = (int64_t)1 << srcLevels;
	bool inside = true;
	for( int i = 0; i < 3; i++ )
	{
		s[i] = resampleFloor( xf.m[3 * i] * q0 + xf.m[3 * i + 1] * q1 + xf.m[3 * i + 2] * q2 + xf.t[i] );
		inside = inside && s[i] >= 0 && s[i] < Rs;
	}
	return inside;
}
// The node of 2^k cells per axis whose lowest cell is c (k <= 21, c a multiple of 2^k, c + 2^k <= 2^21): the exact bounding box of the source cells of all its
// sample points, clipped to [0, 2^srcLevels)^3.  Per axis the extremes of a sum of three terms linear in one coordinate each are the sums of the terms' extremes,
// taken at the first and the last sample coordinate; floor is monotone.  False when the box misses the source grid on some axis; else lo <= hi, inclusive
MVRT_HDI bool resampleBox( const ResampleXf& xf, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k, uint32_t srcLevels, uint32_t lo[3], uint32_t hi[3] )
{
	const int64_t span = ( (int64_t)1 << k ) - 1, Rs = (int64_t)1 << srcLevels;
	const int64_t qLo[3] = { 2 * (int64_t)c0 + 1, 2 * (int64_t)c1 + 1, 2 * (int64_t)c2 + 1 };
	for( int i = 0; i < 3; i++ )
	{
		int64_t pMin = xf.t[i], pMax = xf.t[i];
		for( int j = 0; j < 3; j++ )
		{
			const int64_t a = xf.m[3 * i + j] * qLo[j], b = xf.m[3 * i + j] * ( qLo[j] + 2 * span );
			pMin += a < b ? a : b;
			pMax += a < b ? b : a;
		}
		const int64_t sMin = resampleFloor( pMin ), sMax = resampleFloor( pMax );
		if( sMax < 0 || sMin >= Rs ) return false;
		lo[i] = (uint32_t)( sMin < 0 ? 0 : sMin );
		hi[i] = (uint32_t)( sMax >= Rs ? Rs - 1 : sMax );
	}
	return true;
}
// the smallest h at which the box [lo, hi] spans at most 2 cells of 2^h per axis: at most 8 coarse cells cover it (h <= the levels of the grid the box lies in)
MVRT_HDI uint32_t resampleBoxShift( const uint32_t lo[3], const uint32_t hi[3] )
{
	uint32_t h = 0;
	while( ( hi[0] >> h ) - ( lo[0] >> h ) > 1u || ( hi[1] >> h ) - ( lo[1] >> h ) > 1u || ( hi[2] >> h ) - ( lo[2] >> h ) > 1u ) h++;
	return h;
}
// whether one of the n sorted codes lies in one of the coarse cells that cover the box: per coarse cell one search, a voxel is there when the first code not below
// the cell's first is below the next cell's first ( ( code + 1 ) << 3h <= 2^63 ).  Conservative: the cover may be larger than the box, never smaller
MVRT_HDI bool resampleBoxHoldsVoxel( const uint64_t* __restrict__ codes, uint64_t n, const uint32_t lo[3], const uint32_t hi[3] )
{
	const uint32_t h = resampleBoxShift( lo, hi ), shift = 3u * h;
	const uint32_t x0 = lo[0] >> h, y0 = lo[1] >> h, z0 = lo[2] >> h, nx = ( hi[0] >> h ) - x0, ny = ( hi[1] >> h ) - y0, nz = ( hi[2] >> h ) - z0;
	for( uint32_t dz = 0; dz <= nz; dz++ )
		for( uint32_t dy = 0; dy <= ny; dy++ )
			for( uint32_t dx = 0; dx <= nx; dx++ )
			{
				const uint64_t code = mortonEncode( x0 + dx, y0 + dy, z0 + dz );
				const uint64_t i = lowerBound( codes, 0, n, code << shift );
				if( i < n && codes[i] < ( code + 1ull ) << shift ) return true;
			}
	return false;
}

// ---- union-find over node ids (kernels_fill.hip, kernels_components.hip) --------------------------------------------------------------------------------------
// parent[v] <= v always, a root has parent[v] == v, only roots are ever hooked and only under smaller ids: the root of a set is its lowest id whatever the
// schedule.  Nothing here waits on another thread: find() walks strictly downwards in id (a parent is never larger than its child), unite() retries only after a
// failed compare-and-swap, and then from a strictly smaller id.  Device only.
MVRT_DI uint32_t ufLoad( uint32_t* p ) { return __hip_atomic_load( p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ); }
MVRT_DI void ufStore( uint32_t* p, uint32_t v ) { __hip_atomic_store( p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ); }
// v strictly decreases.  Path halving on the way: a node that is no root (it never becomes one again) is pointed at its grandparent, an ancestor with a lower id
MVRT_DI uint32_t ufFind( uint32_t* parent, uint32_t v )
{
	for( ;; )
	{
		const uint32_t p = ufLoad( parent + v );
		if( p >= v ) return v; // ( p == v: a root )
		const uint32_t gp = ufLoad( parent + p );
		if( gp < p ) ufStore( parent + v, gp );
		v = p;
	}
}
MVRT_DI void ufUnite( uint32_t* parent, uint32_t a, uint32_t b )
{
	for( ;; )
	{
		a = ufFind( parent, a );
		b = ufFind( parent, b );
		if( a == b ) return;
		if( a < b )
		{
			const uint32_t t = a;
			a = b;
			b = t;
		}
		// a > b: hook a under b if a is still a root.  Otherwise somebody hooked it meanwhile, under an id below a: the next find( a ) ends lower, so a + b
		// strictly decreases from one turn to the next
		if( atomicCAS( parent + a, a, b ) == a ) return;
	}
}
// the same walk without the stores, for a flatten: there parent[v] is written once, by v's own thread, with the root
MVRT_DI uint32_t ufRoot( uint32_t* parent, uint32_t v )
{
	for( ;; )
	{
		const uint32_t p = ufLoad( parent + v );
		if( p >= v ) return v;
		v = p;
	}
}

// ---- wave reductions --------------------------------------------------------------------------------------------------------------------------------------
// All 64 lanes of the wave call these; lane 0 ends with the sum, the maximum or the minimum of the wave's values.  The Into forms are the usual end of a counting
// kernel: lane 0 adds (or maximises) a result that is not 0 into a 64-bit counter, one atomic per wave.  T is the type the shuffles move.  Device only.
template <class T> MVRT_DI T waveSum( T v )
{
	for( int o = 32; o > 0; o >>= 1 ) v += __shfl_down( v, o, 64 );
	return v;
}
template <class T> MVRT_DI T waveMax( T v )
{
	for( int o = 32; o > 0; o >>= 1 )
	{
		const T w = __shfl_down( v, o, 64 );
		v = w > v ? w : v;
	}
	return v;
}
template <class T> MVRT_DI T waveMin( T v )
{
	for( int o = 32; o > 0; o >>= 1 )
	{
		const T w = __shfl_down( v, o, 64 );
		v = w < v ? w : v;
	}
	return v;
}
MVRT_DI bool waveLane0() { return ( threadIdx.x & 63u ) == 0; }
template <class T> MVRT_DI void waveAddInto( unsigned long long* dst, T v )
{
	v = waveSum( v );
	if( waveLane0() && v ) atomicAdd( dst, (unsigned long long)v );
}
template <class T> MVRT_DI void waveMaxInto( unsigned long long* dst, T v )
{
	v = waveMax( v );
	if( waveLane0() && v ) atomicMax( dst, (unsigned long long)v );
}

// ---- host steps -------------------------------------------------------------------------------------------------------------------------------------------
// offs (allocated here) = the exclusive sums of `items` values of `in`, as T.  lastOnHost: where offs[items - 1] goes, valid when this returns (null = not wanted)
template <class T, class In> int exclusiveOffsets( In in, uint64_t items, DevBuf& offs, T* lastOnHost, hipStream_t st )
{
	if( offs.alloc( items * sizeof( T ) ) ) return 1;
	return withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
		const hipError_t e = hipcub::DeviceScan::ExclusiveSum( tmp, tmpBytes, in, offs.as<T>(), items, st );
		if( e != hipSuccess || !tmp || !lastOnHost ) return e;
		return hipMemcpyAsync( lastOnHost, offs.as<T>() + ( items - 1 ), sizeof( T ), hipMemcpyDeviceToHost, st ); // (withCubTemp waits)
	} );
}
// the same over a functor of the item's number: in = f( 0 ), f( 1 ), ..., the counting and the transform iterator built here (Index: the argument type of f)
template <class T, class Index = uint32_t, class F> int exclusiveOffsetsOf( F f, uint64_t items, DevBuf& offs, T* lastOnHost, hipStream_t st )
{
	typedef hipcub::CountingInputIterator<Index> Counting;
	return exclusiveOffsets<T>( hipcub::TransformInputIterator<T, F, Counting>( Counting( (Index)0 ), f ), items, offs, lastOnHost, st );
}
// n (key, value) pairs sorted by bits [0, endBit) of the key from A into B (allocated here); A is released
inline int sortPairsInto( DevBuf& keysA, DevBuf& valsA, uint64_t n, int endBit, DevBuf& keysB, DevBuf& valsB, hipStream_t st )
{
	if( keysB.alloc( n * 8 ) || valsB.alloc( n * 4 ) ) return 1;
	if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
			return hipcub::DeviceRadixSort::SortPairs( tmp, tmpBytes, keysA.as<uint64_t>(), keysB.as<uint64_t>(), valsA.as<uint32_t>(), valsB.as<uint32_t>(), n, 0, endBit, st );
		} ) )
		return 1;
	keysA.release();
	valsA.release();
	return 0;
}
// rank1 (allocated here) = the inclusive sums of n >= 1 head flags: rank1[i] - 1 is the number of the run entry i lies in.  count: where the number of heads
// goes, valid when this returns (null = not wanted)
template <class In> int rankHeads( In heads, uint64_t n, DevBuf& rank1, uint32_t* count, hipStream_t st )
{
	if( rank1.alloc( n * 4 ) ) return 1;
	return withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
		const hipError_t e = hipcub::DeviceScan::InclusiveSum( tmp, tmpBytes, heads, rank1.as<uint32_t>(), n, st );
		if( e != hipSuccess || !tmp || !count ) return e;
		return hipMemcpyAsync( count, rank1.as<uint32_t>() + ( n - 1 ), 4, hipMemcpyDeviceToHost, st ); // (withCubTemp waits)
	} );
}
// the same over a functor of the entry's number, as exclusiveOffsetsOf
template <class F> int rankHeadsOf( F f, uint64_t n, DevBuf& rank1, uint32_t* count, hipStream_t st )
{
	typedef hipcub::CountingInputIterator<uint32_t> Counting;
	return rankHeads( hipcub::TransformInputIterator<uint32_t, F, Counting>( Counting( 0u ), f ), n, rank1, count, st );
}
// the head flag of sorted keys, for rankHeadsOf: 1 where key i differs from its predecessor (the sorted records of a morphology step and of a band pass, the
// sorted corner keys of the weld)
struct KeyHead
{
	const uint64_t* keys;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return i == 0u || keys[i] != keys[i - 1u] ? 1u : 0u; }
};

// The 64-bit counters of one call, which its kernels add into: allocated and zeroed on the stream by init (slot `ones`, where given, preset to ~0 for a minimum);
// read copies them to the host behind the launches issued so far and waits for the stream
struct Counters
{
	DevBuf buf;
	unsigned long long* dev() const { return buf.as<unsigned long long>(); }
	int init( uint32_t slots, hipStream_t st, int ones = -1 )
	{
		if( buf.alloc( slots * 8 ) ) return 1;
		MVRT_HIP( hipMemsetAsync( buf.p, 0, slots * 8, st ) );
		if( ones >= 0 ) MVRT_HIP( hipMemsetAsync( dev() + ones, 0xFF, 8, st ) );
		return 0;
	}
	int read( unsigned long long* host, uint32_t slots, hipStream_t st ) const
	{
		MVRT_HIP( hipMemcpyAsync( host, buf.p, slots * 8, hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
		return 0;
	}
};
