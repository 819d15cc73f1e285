// kernels_components.hip -- the connected components of the voxel set (mvrt_svo_components / mvrt_svo_keep_components, mvrt.h).  The work grows
// with the number of voxels, never with the number of cells of the grid; everything is integer and a property of the set alone, whatever the schedule.
//
//   unite    node v = voxel v of the sorted codes (vIndex).  One thread per voxel looks at the half of the element whose offsets lie below (0, 0, 0)
//            (componentHalf, voxel_passes.h: 3 of 6, 13 of 26), so every adjacent pair is seen once; a neighbour inside the grid is searched in the codes
//            (codeIndexIn) and, where it is a voxel, united with v.  The union-find is the one of kernels_fill.hip (voxel_passes.h), and what keeps it from
//            ever hanging holds here verbatim: a parent is never larger than its child; only roots are hooked, and only under smaller ids; find() walks
//            strictly downwards; unite() retries only after a failed compare-and-swap, and then from a strictly smaller id; no thread ever waits for another.
//   flatten  a kernel of its own behind the unions, without path halving (the reason stands above kFillFlatten): parent[v] = the root of v = the lowest vIndex of
//            its component, which is the component's `first`.  One inclusive scan of the root flags (rankHeads) numbers the components in order of first
//            appearance: label[v] = rank1[root[v]] - 1.
//   reduce   size by atomicAdd, box by atomicMin / atomicMax on uint32, aggregated in the wave first: the lanes that share the label of the first remaining lane
//            are picked by a ballot, reduced by shuffles, and one lane issues one atomic per output -- for the box only where a load shows that the bound
//            moves.  Every turn retires at least that first lane.  Nearly all voxels of a real scene belong to one component: per-voxel atomics would
//            serialise on one address.
//   select   (in place) the keys ( ~size ) << 32 | label radix-sorted: position = rank by (size descending, label ascending).  One keep flag per component,
//            gathered per voxel as a drop mask, then the erosion's scan and scatter (compactUnmasked, kernels_list.hip).
// No LDS beyond hipcub's, no floating point.
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define CB 256 // threads per workgroup

namespace
{
__global__ void __launch_bounds__( CB ) kCompInitParents( uint32_t* __restrict__ parent, uint32_t n )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( i < n ) parent[i] = (uint32_t)i;
}
__global__ void __launch_bounds__( CB ) kCompUnite( const uint64_t* __restrict__ codes, uint32_t n, uint32_t levels, int element, uint32_t* parent )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( i >= n ) return;
	uint32_t x, y, z;
	mortonDecode( codes[i], x, y, z );
	const uint32_t nb = morphNeighbours( element );
	for( uint32_t j = 0; j < nb; j++ )
	{
		uint64_t c;
		if( !componentHalf( element, j ) || !morphNeighbour( x, y, z, levels, element, j, &c ) ) continue;
		const uint64_t k = codeIndexIn( codes, n, c );
		if( k < n ) ufUnite( parent, (uint32_t)i, (uint32_t)k );
	}
}
// parent[v] = the root of v; the unions are complete (this is a kernel of its own).  No path halving here: a halving store of a grandparent read earlier could
// land behind the store of the root and leave a node that is no root in a flattened entry.  A thread that walks through an entry another thread has flattened
// already reads the root there, else an ancestor as before
__global__ void __launch_bounds__( CB ) kCompFlatten( uint32_t* parent, uint32_t n )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( i >= n ) return;
	const uint32_t v = (uint32_t)i, r = ufRoot( parent, v );
	if( r != v ) ufStore( parent + v, r );
}
struct RootFlag // scan input: 1 where voxel v is the root, the first voxel, of its component
{
	const uint32_t* root;
	__host__ __device__ uint32_t operator()( uint32_t v ) const { return root[v] == v ? 1u : 0u; }
};

// size[c] += the voxels of component c, box[c] = their bounds (min x, y, z, max x, y, z; preset to ~0 and 0; null = not wanted).  The loop runs in every lane of
// the wave, the ones past the end included: `todo` is the same in all of them and loses the leader's bit, at least, every turn
__global__ void __launch_bounds__( CB ) kCompReduce( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank1, uint32_t n,
													 uint32_t* __restrict__ size, uint32_t* box )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	const bool active = i < n;
	const uint32_t label = active ? rank1[root[i]] - 1u : 0u;
	uint32_t p[3] = { 0u, 0u, 0u };
	if( active && box ) mortonDecode( codes[i], p[0], p[1], p[2] );
	const int lane = (int)( threadIdx.x & ( WAVE - 1 ) );
	unsigned long long todo = __ballot( active );
	while( todo )
	{
		const int leader = __ffsll( todo ) - 1;
		const uint32_t l = __shfl( label, leader, WAVE );
		const bool mine = active && label == l;
		const unsigned long long m = __ballot( mine );
		uint32_t lo[3], hi[3];
#pragma unroll
		for( int a = 0; a < 3; a++ )
		{
			lo[a] = mine ? p[a] : ~0u;
			hi[a] = mine ? p[a] : 0u;
		}
		if( box && ( m & ( m - 1ull ) ) ) // more than one lane: the bounds over the wave, the other lanes neutral
			for( int o = WAVE / 2; o > 0; o >>= 1 )
#pragma unroll
				for( int a = 0; a < 3; a++ )
				{
					lo[a] = min( lo[a], __shfl_xor( lo[a], o, WAVE ) );
					hi[a] = max( hi[a], __shfl_xor( hi[a], o, WAVE ) );
				}
		if( lane == leader )
		{
			atomicAdd( size + l, (uint32_t)__popcll( m ) );
			if( box )
#pragma unroll
				for( int a = 0; a < 3; a++ ) // a bound only ever moves outwards, so a value read earlier is no tighter than the current one: nothing needed is skipped
				{
					uint32_t* b = box + (uint64_t)l * 6u + a;
					if( lo[a] < ufLoad( b ) ) atomicMin( b, lo[a] );
					if( hi[a] > ufLoad( b + 3 ) ) atomicMax( b + 3, hi[a] );
				}
		}
		todo &= ~m;
	}
}
__global__ void __launch_bounds__( CB ) kCompInitBox( uint32_t* __restrict__ box, uint32_t nComponents )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( i < (uint64_t)nComponents * 6u ) box[i] = i % 6u < 3u ? ~0u : 0u;
}
__global__ void __launch_bounds__( CB ) kCompLargest( const uint32_t* __restrict__ size, uint32_t nComponents, uint32_t* __restrict__ largest )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	uint32_t s = i < nComponents ? size[i] : 0u;
	for( int o = WAVE / 2; o > 0; o >>= 1 ) s = max( s, __shfl_xor( s, o, WAVE ) );
	if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicMax( largest, s );
}
// the listing's per-voxel and per-root outputs; either may be null
__global__ void __launch_bounds__( CB ) kCompList( const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank1, uint32_t n, uint32_t* __restrict__ label,
												   uint32_t* __restrict__ first )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( i >= n ) return;
	const uint32_t r = root[i];
	if( label ) label[i] = rank1[r] - 1u;
	if( first && r == (uint32_t)i ) first[rank1[r] - 1u] = r;
}

// ---- selection -----------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__( CB ) kCompKeys( const uint32_t* __restrict__ size, uint32_t nComponents, uint64_t* __restrict__ keys )
{
	const uint64_t c = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( c < nComponents ) keys[c] = (uint64_t)( ~size[c] ) << 32 | c;
}
// sorted: the keys in ascending order, position = rank.  keep[label] = 1 where the component stays; the kept ones are counted, one atomic per wave
__global__ void __launch_bounds__( CB ) kCompKeep( const uint64_t* __restrict__ sorted, uint32_t nComponents, uint64_t minVoxels, uint32_t keepLargest, uint32_t* __restrict__ keep,
												   uint32_t* __restrict__ nKept )
{
	const uint64_t r = (uint64_t)blockIdx.x * CB + threadIdx.x;
	bool k = false;
	if( r < nComponents )
	{
		const uint64_t key = sorted[r];
		const uint32_t size = ~(uint32_t)( key >> 32 );
		k = size >= minVoxels && ( keepLargest == 0u || r < keepLargest );
		keep[(uint32_t)key] = k ? 1u : 0u;
	}
	const unsigned long long m = __ballot( k );
	if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 && m ) atomicAdd( nKept, (uint32_t)__popcll( m ) );
}
// drop[v] = 1 where the component of voxel v goes: the mask of the erosion's compaction
__global__ void __launch_bounds__( CB ) kCompDropMask( const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank1, const uint32_t* __restrict__ keep, uint32_t n,
													   uint32_t* __restrict__ drop )
{
	const uint64_t i = (uint64_t)blockIdx.x * CB + threadIdx.x;
	if( i < n ) drop[i] = keep[rank1[root[i]] - 1u] ? 0u : 1u;
}

// what the labelling leaves: root[v] = the first voxel of v's component, rank1[v] = the roots up to and including v.  Has waited for the stream
struct Labelled
{
	DevBuf root, rank1;
	uint32_t nComponents = 0;
};
int labelComponents( const SurfaceSource& s, int element, Labelled* out, hipStream_t st )
{
	const uint32_t n = s.nVoxels;
	const dim3 grid( divUp( n, CB ) ), block( CB );
	if( out->root.alloc( (uint64_t)n * 4 ) ) return 1;
	uint32_t* parent = out->root.as<uint32_t>();
	hipLaunchKernelGGL( kCompInitParents, grid, block, 0, st, parent, n );
	hipLaunchKernelGGL( kCompUnite, grid, block, 0, st, s.morton, n, s.levels, element, parent );
	hipLaunchKernelGGL( kCompFlatten, grid, block, 0, st, parent, n );
	MVRT_HIP( hipGetLastError() );
	return rankHeadsOf( RootFlag{ parent }, n, out->rank1, &out->nComponents, st );
}
// size (allocated here, and box where wanted) of every component.  Not synchronised
int reduceComponents( const SurfaceSource& s, const Labelled& l, DevBuf& size, DevBuf* box, hipStream_t st )
{
	const uint32_t nc = l.nComponents;
	if( size.alloc( (uint64_t)nc * 4 ) || ( box && box->alloc( (uint64_t)nc * 24 ) ) ) return 1;
	MVRT_HIP( hipMemsetAsync( size.p, 0, (uint64_t)nc * 4, st ) );
	if( box ) hipLaunchKernelGGL( kCompInitBox, dim3( divUp( (uint64_t)nc * 6, CB ) ), dim3( CB ), 0, st, box->as<uint32_t>(), nc );
	hipLaunchKernelGGL( kCompReduce, dim3( divUp( s.nVoxels, CB ) ), dim3( CB ), 0, st, s.morton, l.root.as<uint32_t>(), l.rank1.as<uint32_t>(), s.nVoxels, size.as<uint32_t>(),
						box ? box->as<uint32_t>() : nullptr );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
} // namespace

int componentsList( const SurfaceSource& s, int element, uint32_t* labelDev, uint64_t capacity, uint32_t* sizeDev, uint32_t* firstDev, uint32_t* boxDev, uint64_t* nComponentsOut,
					uint64_t* largestOut, hipStream_t st )
{
	Labelled l;
	if( labelComponents( s, element, &l, st ) ) return 1;
	const uint32_t nc = l.nComponents;
	const bool fits = capacity >= nc;
	DevBuf size, box, count;
	if( reduceComponents( s, l, size, boxDev && fits ? &box : nullptr, st ) || count.alloc( 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( count.p, 0, 4, st ) );
	hipLaunchKernelGGL( kCompLargest, dim3( divUp( nc, CB ) ), dim3( CB ), 0, st, size.as<uint32_t>(), nc, count.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	uint32_t largest = 0;
	MVRT_HIP( hipMemcpyAsync( &largest, count.p, 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	if( nComponentsOut ) *nComponentsOut = nc;
	if( largestOut ) *largestOut = largest;
	if( !labelDev && !sizeDev && !firstDev && !boxDev ) return 0; // the sizing call
	if( !fits && ( sizeDev || firstDev || boxDev ) )
	{
		listingRefusal( "mvrt_svo_components", "componentCapacity", "components", capacity, nc );
		return 1;
	}
	// (the caller's arrays are written from here on, behind every allocation and check)
	if( labelDev || firstDev )
	{
		hipLaunchKernelGGL( kCompList, dim3( divUp( s.nVoxels, CB ) ), dim3( CB ), 0, st, l.root.as<uint32_t>(), l.rank1.as<uint32_t>(), s.nVoxels, labelDev, firstDev );
		MVRT_HIP( hipGetLastError() );
	}
	if( sizeDev ) MVRT_HIP( hipMemcpyAsync( sizeDev, size.p, (uint64_t)nc * 4, hipMemcpyDeviceToDevice, st ) );
	if( boxDev ) MVRT_HIP( hipMemcpyAsync( boxDev, box.p, (uint64_t)nc * 24, hipMemcpyDeviceToDevice, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int componentsKeepList( const SurfaceSource& s, int element, uint64_t minVoxels, uint32_t keepLargest, SortedVoxels& out, uint32_t* nComponents, uint32_t* nKeptComponents,
						hipStream_t st )
{
	Labelled l;
	if( labelComponents( s, element, &l, st ) ) return 1;
	const uint32_t nc = l.nComponents;
	*nComponents = nc;
	out.n = s.nVoxels;
	out.hasEmission = 0;
	DevBuf drop;
	{
		DevBuf size, keys, sorted, keep, count;
		if( reduceComponents( s, l, size, nullptr, st ) || keys.alloc( (uint64_t)nc * 8 ) || sorted.alloc( (uint64_t)nc * 8 ) ) return 1;
		const dim3 grid( divUp( nc, CB ) ), block( CB );
		hipLaunchKernelGGL( kCompKeys, grid, block, 0, st, size.as<uint32_t>(), nc, keys.as<uint64_t>() );
		MVRT_HIP( hipGetLastError() );
		if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
				return hipcub::DeviceRadixSort::SortKeys( tmp, tmpBytes, keys.as<uint64_t>(), sorted.as<uint64_t>(), (uint64_t)nc, 0, 64, st );
			} ) )
			return 1;
		if( keep.alloc( (uint64_t)nc * 4 ) || count.alloc( 4 ) ) return 1;
		MVRT_HIP( hipMemsetAsync( count.p, 0, 4, st ) );
		hipLaunchKernelGGL( kCompKeep, grid, block, 0, st, sorted.as<uint64_t>(), nc, minVoxels, keepLargest, keep.as<uint32_t>(), count.as<uint32_t>() );
		MVRT_HIP( hipGetLastError() );
		MVRT_HIP( hipMemcpyAsync( nKeptComponents, count.p, 4, hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
		if( *nKeptComponents == nc ) return 0; // nothing goes
		if( *nKeptComponents == 0 )
		{
			out.n = 0;
			return 0; // (the caller refuses)
		}
		if( drop.alloc( (uint64_t)s.nVoxels * 4 ) ) return 1;
		hipLaunchKernelGGL( kCompDropMask, dim3( divUp( s.nVoxels, CB ) ), block, 0, st, l.root.as<uint32_t>(), l.rank1.as<uint32_t>(), keep.as<uint32_t>(), s.nVoxels,
							drop.as<uint32_t>() );
		MVRT_HIP( hipGetLastError() );
		MVRT_HIP( hipStreamSynchronize( st ) ); // (keep is released at scope end)
	}
	l = Labelled();
	return compactUnmasked( s.morton, s.attrs, drop.as<uint32_t>(), s.nVoxels, true, out, st );
}
