// kernels_fill.hip -- the enclosed empty cells of the voxel set (mvrt_svo_enclosed_cells / mvrt_svo_fill_enclosed / mvrt_svo_surface_exterior_masks, mvrt.h).  The work grows with
// the number of voxels, never with the number of cells of the grid.
//
//   rows    the voxels sorted by the linear key ( z * R + y ) * R + x (one radix sort of the codes): a row is one (y, z), its voxels lie together by x.
//   gaps    gap i = the empty run between sorted voxels i and i + 1 where they share a row and their x differ by more than 1.  The run before the first voxel of
//           a row, the run behind its last one and every row without voxels hold a border cell: exterior by themselves.  Only a gap can be enclosed.
//   unions  node 0 = EXTERIOR, node i + 1 = gap i.  One thread per gap looks at its four neighbour rows (y +- 1, z), (y, z +- 1): a row outside the grid joins the
//           gap to EXTERIOR; in a row inside it a binary search finds the first voxel at or behind the gap's x0 and a walk up to x1 unites the gap with every
//           gap it overlaps and with EXTERIOR for every overlapped stretch that is an end run or a voxel-free row.  The larger root is always hooked under the
//           smaller one: the root of a set is its lowest id whatever the schedule, and EXTERIOR is the root of everything exterior.
//   emit    flatten, length of every gap whose root is not EXTERIOR, 64-bit exclusive scan, then the run expansion of voxel_passes.h: one workgroup per 256 gaps
//           writes its cells, one thread per cell; radix sort of (Morton code, root), roots ranked by the position of their first cell (sortPairsInto, rankHeads).
//
//   exterior  the front half alone -- rows, unions, flatten -- serves mvrt_svo_surface_exterior_masks: the plain exposure masks of
//           kernels_surface.hip, then one pass that clears every bit whose neighbour cell lies in a gap with a root other than EXTERIOR.
//
// Nothing here waits on another thread.  find() walks strictly downwards in id (a parent is never larger than its child), unite() retries only after a failed
// compare-and-swap, and then from a strictly smaller id; the neighbour walk advances its voxel index every turn.
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define FB 256 // threads per workgroup, and gaps per workgroup of the emit kernel

namespace
{
__global__ void __launch_bounds__( FB ) kFillLinearKeys( const uint64_t* __restrict__ morton, uint32_t n, uint32_t L, uint64_t* __restrict__ keys )
{
	const uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x;
	if( i >= n ) return;
	uint32_t x, y, z;
	mortonDecode( morton[i], x, y, z );
	keys[i] = ( (uint64_t)z << ( 2u * L ) ) | ( (uint64_t)y << L ) | x;
}

// (gapLength and gapNodeOfCell: voxel_passes.h)

// (ufLoad, ufStore, ufFind, ufUnite and ufRoot, the union-find over node ids: voxel_passes.h)

__global__ void __launch_bounds__( FB ) kFillInitParents( uint32_t* __restrict__ parent, uint64_t nNodes )
{
	const uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x;
	if( i < nNodes ) parent[i] = (uint32_t)i;
}

// gap g = [x0, x1] of some row against the row `row` (= z << L | y, inside the grid)
MVRT_DI void uniteWithRow( const uint64_t* __restrict__ lin, uint32_t n, uint32_t L, uint32_t* parent, uint32_t g, uint64_t row, uint64_t x0, uint64_t x1 )
{
	const uint64_t xMask = ( 1ull << L ) - 1ull;
	uint64_t j = lowerBound( lin, 0, n, ( row << L ) | x0 ); // the first voxel of the list at or behind (row, x0)
	uint64_t cur = x0;										 // the first cell of [x0, x1] not yet looked at
	bool leftVoxel = j > 0 && ( lin[j - 1] >> L ) == row;	 // is there a voxel of this row left of cur?
	for( ;; j++ )											 // j < n grows every turn
	{
		const bool inRow = j < n && ( lin[j] >> L ) == row;
		const uint64_t xj = inRow ? ( lin[j] & xMask ) : ~0ull;
		const uint64_t end = inRow && xj <= x1 ? xj : x1 + 1; // the empty stretch [cur, end) lies within [x0, x1]
		if( end > cur ) ufUnite( parent, g, leftVoxel && inRow ? (uint32_t)j : 0u ); // between voxels j - 1 and j of one row: gap j - 1 = node j; else an end run or a voxel-free row
		if( !inRow || xj >= x1 ) return;
		cur = xj + 1;
		leftVoxel = true;
	}
}

__global__ void __launch_bounds__( FB ) kFillUnite( const uint64_t* __restrict__ lin, uint32_t n, uint32_t L, uint32_t* parent )
{
	const uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x;
	const uint64_t len = gapLength( lin, n, L, i );
	if( len == 0 ) return;
	const uint64_t R = 1ull << L, xMask = R - 1ull;
	const uint64_t a = lin[i];
	const uint64_t row = a >> L, y = row & xMask, z = row >> L;
	const uint64_t x0 = ( a & xMask ) + 1ull, x1 = x0 + len - 1ull;
	const uint32_t g = (uint32_t)i + 1u;
	if( y == 0 || y == R - 1 || z == 0 || z == R - 1 ) ufUnite( parent, g, 0u ); // a neighbour row outside the grid (and the gap's own cells are border cells)
	if( y > 0 ) uniteWithRow( lin, n, L, parent, g, row - 1ull, x0, x1 );
	if( y < R - 1 ) uniteWithRow( lin, n, L, parent, g, row + 1ull, x0, x1 );
	if( z > 0 ) uniteWithRow( lin, n, L, parent, g, row - R, x0, x1 );
	if( z < R - 1 ) uniteWithRow( lin, n, L, parent, g, row + R, x0, x1 );
}

// parent[v] = the root of v (node v = gap v - 1; the unions are complete: this is a kernel of its own), and the number of enclosed regions = gaps that are
// their own root.  No path halving here: a halving store of a grandparent read earlier could land behind the store of the root and leave a node that is no
// root in a flattened entry.  A thread that walks through an entry another thread has flattened already reads the root there, else an ancestor as before
__global__ void __launch_bounds__( FB ) kFillFlatten( const uint64_t* __restrict__ lin, uint32_t n, uint32_t L, uint32_t* parent, unsigned long long* __restrict__ nRegions )
{
	const uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x;
	uint32_t isRoot = 0;
	if( i < n && gapLength( lin, n, L, i ) )
	{
		const uint32_t g = (uint32_t)i + 1u;
		const uint32_t r = ufRoot( parent, g );
		if( r != g ) ufStore( parent + g, r );
		isRoot = r == g ? 1u : 0u;
	}
	const unsigned long long m = __ballot( isRoot );
	if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 && m ) atomicAdd( nRegions, (unsigned long long)__popcll( m ) );
}

// ---- exterior masks (mvrt_svo_surface_exterior_masks) --------------------------------------------------------------------------------------------
// masks: the plain exposure masks in vIndex order, changed in place: a set bit whose neighbour cell lies inside the grid and in a gap whose root is not EXTERIOR
// is cleared.  One thread per voxel, the owner of its byte.  The +-X neighbours share the voxel's row: one search of its own key gives its rank p in lin, they
// are the gaps p and p - 1 where those exist; the other four directions take one search each (gapNodeOfCell).  A neighbour that is no gap cell maps to node 0,
// whose root is 0.  The cleared bits are counted by a wave reduction and one atomic per wave.
__global__ void __launch_bounds__( FB ) kFillExteriorMasks( const uint64_t* __restrict__ morton, const uint64_t* __restrict__ lin, const uint32_t* __restrict__ root, uint32_t n, uint32_t L,
															uint8_t* __restrict__ masks, unsigned long long* __restrict__ nHidden )
{
	const uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x;
	uint32_t cleared = 0;
	const uint32_t m = i < n ? masks[i] : 0u;
	if( m )
	{
		uint32_t x, y, z;
		mortonDecode( morton[i], x, y, z );
		const uint32_t last = ( 1u << L ) - 1u; // R - 1
		const uint64_t row = ( (uint64_t)z << L ) | y, key = ( row << L ) | x;
		uint32_t node[6] = { 0u, 0u, 0u, 0u, 0u, 0u }; // per direction; 0 = outside the grid, no face, or no gap
		if( ( m & 0x28u ) != 0u ) // +X or -X
		{
			const uint64_t p = lowerBound( lin, 0, n, key ); // ( lin[p] == key )
			if( ( m & 0x08u ) && x < last && p + 1 < n && ( lin[p + 1] >> L ) == row ) node[3] = (uint32_t)p + 1u; // gap p
			if( ( m & 0x20u ) && x > 0u && p > 0 && p < n && ( lin[p - 1] >> L ) == row ) node[5] = (uint32_t)p;	   // gap p - 1
		}
		if( ( m & 0x01u ) && y > 0u ) node[0] = gapNodeOfCell( lin, n, L, key - ( 1ull << L ) );
		if( ( m & 0x02u ) && y < last ) node[1] = gapNodeOfCell( lin, n, L, key + ( 1ull << L ) );
		if( ( m & 0x04u ) && z > 0u ) node[2] = gapNodeOfCell( lin, n, L, key - ( 1ull << ( 2u * L ) ) );
		if( ( m & 0x10u ) && z < last ) node[4] = gapNodeOfCell( lin, n, L, key + ( 1ull << ( 2u * L ) ) );
		uint32_t out = m;
#pragma unroll
		for( uint32_t d = 0; d < 6; d++ )
			if( node[d] != 0u && root[node[d]] != 0u ) out &= ~( 1u << d );
		cleared = __popc( m ^ out );
		if( cleared ) masks[i] = (uint8_t)out;
	}
	waveAddInto( nHidden, cleared );
}

struct EnclosedLength // scan input: the cells of gap i where its root is not EXTERIOR (item n - 1 and beyond: 0)
{
	const uint64_t* lin;
	const uint32_t* root;
	uint32_t n, L;
	__host__ __device__ uint64_t operator()( uint32_t i ) const
	{
		const uint64_t len = gapLength( lin, n, L, i );
		return len && root[i + 1u] != 0u ? len : 0ull;
	}
};

// One workgroup per FB gaps, the run expansion of voxel_passes.h: offs = n + 1 exclusive offsets (offs[n] = nCells), the records are cells, a gap's cells its x in order.
// codes / roots: the (Morton code, root) pairs of the listing; xyz: the coordinates as they come (the fill, which sorts them itself).  Either may be null.
__global__ void __launch_bounds__( FB ) kFillEmit( const uint64_t* __restrict__ lin, const uint32_t* __restrict__ root, const uint64_t* __restrict__ offs, uint32_t n, uint32_t L,
												   uint64_t* __restrict__ codes, uint32_t* __restrict__ roots, uint32_t* __restrict__ xyz )
{
	__shared__ uint32_t sOff[FB + 1];
	__shared__ uint64_t sLin[FB];
	__shared__ uint32_t sRoot[FB];
	const uint64_t v = (uint64_t)blockIdx.x * FB + threadIdx.x;
	const uint64_t base = stageRunOffsets<FB>( offs, n, sOff ); // (relative offsets <= FB * 2^21)
	sLin[threadIdx.x] = v < n ? lin[v] : 0ull;
	sRoot[threadIdx.x] = v < n ? root[v + 1] : 0u;
	__syncthreads();
	const uint32_t total = sOff[FB];
	const uint64_t xMask = ( 1ull << L ) - 1ull;
	for( uint32_t j = threadIdx.x; j < total; j += FB )
	{
		const uint32_t lo = findRun( sOff, FB, j );
		const uint64_t a = sLin[lo];
		const uint32_t x = (uint32_t)( a & xMask ) + 1u + ( j - sOff[lo] ), y = (uint32_t)( ( a >> L ) & xMask ), z = (uint32_t)( a >> ( 2u * L ) );
		const uint64_t c = base + j;
		if( codes )
		{
			codes[c] = mortonEncode( x, y, z );
			roots[c] = sRoot[lo];
		}
		if( xyz )
		{
			xyz[c * 3] = x;
			xyz[c * 3 + 1] = y;
			xyz[c * 3 + 2] = z;
		}
	}
}

// the cells sorted by Morton code: firstCell[root] = the lowest position of a cell of that root (preset to ~0).  Only the first cell of a run of equal roots asks
__global__ void __launch_bounds__( FB ) kFillFirstCells( const uint32_t* __restrict__ roots, uint32_t nCells, uint32_t* __restrict__ firstCell )
{
	const uint64_t c = (uint64_t)blockIdx.x * FB + threadIdx.x;
	if( c >= nCells ) return;
	const uint32_t r = roots[c];
	if( c == 0 || roots[c - 1] != r ) atomicMin( firstCell + r, (uint32_t)c );
}
struct RegionHead // scan input: 1 where cell c is the first one of its region
{
	const uint32_t* roots;
	const uint32_t* firstCell;
	__host__ __device__ uint32_t operator()( uint32_t c ) const { return firstCell[roots[c]] == c ? 1u : 0u; }
};
// rank1: the inclusive scan of the heads.  region = rank of the root's first cell; xyz = the decoded code
__global__ void __launch_bounds__( FB ) kFillList( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ roots, const uint32_t* __restrict__ firstCell,
												   const uint32_t* __restrict__ rank1, uint32_t nCells, uint32_t* __restrict__ xyz, uint32_t* __restrict__ region )
{
	const uint64_t c = (uint64_t)blockIdx.x * FB + threadIdx.x;
	if( c >= nCells ) return;
	if( region ) region[c] = rank1[firstCell[roots[c]]] - 1u;
	if( xyz ) mortonDecode( codes[c], xyz[c * 3], xyz[c * 3 + 1], xyz[c * 3 + 2] );
}

__global__ void __launch_bounds__( FB ) kFillAttribs( uint2 attrib, uint64_t n, uint2* __restrict__ out )
{
	const uint64_t i = (uint64_t)blockIdx.x * FB + threadIdx.x;
	if( i < n ) out[i] = attrib;
}

typedef EnclosedClassified Classified; // (launch.h)
// keys, sort, parents, unions, flatten: lin and root.  nRegions is on its way to the host: valid once the stream has been waited for
int classifyGaps( const SurfaceSource& s, Classified* out, hipStream_t st )
{
	const uint32_t n = s.nVoxels, L = s.levels;
	const dim3 grid( divUp( n, FB ) ), block( FB );
	if( out->count.alloc( 8 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( out->count.p, 0, 8, st ) );
	{
		DevBuf keys;
		if( keys.alloc( (uint64_t)n * 8 ) || out->lin.alloc( (uint64_t)n * 8 ) ) return 1;
		hipLaunchKernelGGL( kFillLinearKeys, grid, block, 0, st, s.morton, n, L, keys.as<uint64_t>() );
		MVRT_HIP( hipGetLastError() );
		if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
				return hipcub::DeviceRadixSort::SortKeys( tmp, tmpBytes, keys.as<uint64_t>(), out->lin.as<uint64_t>(), (uint64_t)n, 0, (int)( 3u * L ), st );
			} ) )
			return 1;
	}
	const uint64_t nNodes = (uint64_t)n + 1;
	if( out->root.alloc( nNodes * 4 ) ) return 1;
	hipLaunchKernelGGL( kFillInitParents, dim3( divUp( nNodes, FB ) ), block, 0, st, out->root.as<uint32_t>(), nNodes );
	hipLaunchKernelGGL( kFillUnite, grid, block, 0, st, out->lin.as<uint64_t>(), n, L, out->root.as<uint32_t>() );
	hipLaunchKernelGGL( kFillFlatten, grid, block, 0, st, out->lin.as<uint64_t>(), n, L, out->root.as<uint32_t>(), out->count.as<unsigned long long>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipMemcpyAsync( &out->nRegions, out->count.p, 8, hipMemcpyDeviceToHost, st ) ); // (behind kFillFlatten)
	return 0;
}
// the same and the cell offsets of the enclosed gaps; the scan waits for the stream
int classify( const SurfaceSource& s, Classified* out, hipStream_t st )
{
	if( classifyGaps( s, out, st ) ) return 1;
	return exclusiveOffsetsOf<uint64_t>( EnclosedLength{ out->lin.as<uint64_t>(), out->root.as<uint32_t>(), s.nVoxels, s.levels }, (uint64_t)s.nVoxels + 1, out->offs, &out->nCells,
										 st );
}
int launchEmit( const SurfaceSource& s, const Classified& c, uint64_t* codes, uint32_t* roots, uint32_t* xyz, hipStream_t st )
{
	hipLaunchKernelGGL( kFillEmit, dim3( divUp( s.nVoxels, FB ) ), dim3( FB ), 0, st, c.lin.as<uint64_t>(), c.root.as<uint32_t>(), c.offs.as<uint64_t>(), s.nVoxels, s.levels, codes,
						roots, xyz );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
} // namespace

int enclosedClassify( const SurfaceSource& s, EnclosedClassified* out, hipStream_t st ) { return classify( s, out, st ); }

int enclosedRegionRanks( const uint32_t* roots, uint32_t nCells, uint32_t nVoxels, DevBuf& firstCell, DevBuf& rank1, hipStream_t st )
{
	const uint64_t nNodes = (uint64_t)nVoxels + 1;
	if( firstCell.alloc( nNodes * 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( firstCell.p, 0xFF, nNodes * 4, st ) );
	hipLaunchKernelGGL( kFillFirstCells, dim3( divUp( nCells, FB ) ), dim3( FB ), 0, st, roots, nCells, firstCell.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	return rankHeadsOf( RegionHead{ roots, firstCell.as<uint32_t>() }, nCells, rank1, nullptr, st );
}

int enclosedCells( const SurfaceSource& s, uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint64_t* nCellsOut, uint64_t* nRegionsOut, hipStream_t st )
{
	Classified c;
	if( classify( s, &c, st ) ) return 1;
	if( nCellsOut ) *nCellsOut = c.nCells;
	if( nRegionsOut ) *nRegionsOut = c.nRegions;
	if( !xyzDev && !regionDev ) return 0; // the sizing call
	if( c.nCells >= ( 1ull << 32 ) )
	{
		mvrtSetError( "mvrt_svo_enclosed_cells: the %llu enclosed cells are 2^32 or more, beyond what one listing holds; nothing was written", (unsigned long long)c.nCells );
		return 1;
	}
	const int tail = listingTail( "mvrt_svo_enclosed_cells", "capacity", "enclosed cells", false, capacity, c.nCells );
	if( tail != LISTING_WRITE ) return tail;
	const uint32_t nCells = (uint32_t)c.nCells;
	DevBuf codesA, rootsA, codes, roots, firstCell, rank1;
	if( codesA.alloc( c.nCells * 8 ) || rootsA.alloc( c.nCells * 4 ) ) return 1;
	if( launchEmit( s, c, codesA.as<uint64_t>(), rootsA.as<uint32_t>(), nullptr, st ) ) return 1;
	if( sortPairsInto( codesA, rootsA, c.nCells, (int)( 3u * s.levels ), codes, roots, st ) ) return 1;
	c.lin.release();
	c.offs.release();
	c.root.release();
	if( enclosedRegionRanks( roots.as<uint32_t>(), nCells, s.nVoxels, firstCell, rank1, st ) ) return 1;
	const dim3 grid( divUp( nCells, FB ) ), block( FB );
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	hipLaunchKernelGGL( kFillList, grid, block, 0, st, codes.as<uint64_t>(), roots.as<uint32_t>(), firstCell.as<uint32_t>(), rank1.as<uint32_t>(), nCells, xyzDev, regionDev );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int enclosedCellsUnordered( const SurfaceSource& s, DevBuf& xyz, uint64_t* nCells, hipStream_t st )
{
	Classified c;
	if( classify( s, &c, st ) ) return 1;
	*nCells = c.nCells;
	if( c.nCells == 0 || c.nCells >= ( 1ull << 32 ) ) return 0; // (nothing to list / the caller refuses the count)
	if( xyz.alloc( c.nCells * 12 ) ) return 1;
	if( launchEmit( s, c, nullptr, nullptr, xyz.as<uint32_t>(), st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int surfaceExteriorMasks( const SurfaceSource& s, uint8_t* masksDev, uint64_t* nFacesOut, uint64_t* nHiddenOut, hipStream_t st )
{
	Classified c;
	if( classifyGaps( s, &c, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (nRegions)
	Counters cnt; // [0] plain faces [1] hidden faces
	DevBuf own;
	if( cnt.init( 2, st ) ) return 1;
	uint8_t* masks = masksDev;
	if( !masks && c.nRegions ) // counts only: the second kernel still reads the plain masks
	{
		if( own.alloc( s.nVoxels ) ) return 1;
		masks = own.as<uint8_t>();
	}
	// (the caller's array is written from here on, behind every allocation)
	if( launchSurfaceMasks( s, masks, cnt.dev(), st ) ) return 1;
	if( c.nRegions ) // without an enclosed region the exterior masks are the plain masks
	{
		hipLaunchKernelGGL( kFillExteriorMasks, dim3( divUp( s.nVoxels, FB ) ), dim3( FB ), 0, st, s.morton, c.lin.as<uint64_t>(), c.root.as<uint32_t>(), s.nVoxels, s.levels, masks,
							cnt.dev() + 1 );
		MVRT_HIP( hipGetLastError() );
	}
	unsigned long long h[2] = { 0, 0 };
	if( cnt.read( h, 2, st ) ) return 1; // (waits: the scratch is released on return)
	if( nFacesOut ) *nFacesOut = h[0] - h[1];
	if( nHiddenOut ) *nHiddenOut = h[1];
	return 0;
}

int launchFillAttribs( uint2 attrib, uint64_t n, uint2* out, hipStream_t st )
{
	hipLaunchKernelGGL( kFillAttribs, dim3( divUp( n, FB ) ), dim3( FB ), 0, st, attrib, n, out );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
