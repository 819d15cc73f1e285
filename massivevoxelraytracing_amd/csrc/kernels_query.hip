// kernels_query.hip -- the nearest voxel of arbitrary lattice points (mvrt_svo_nearest_voxels), of every voxel of a second set (mvrt_svo_nearest_between) and the
// recolouring of one set from another (mvrt_svo_transfer_attributes); mvrt.h, DESIGN.md 5.24.
//
//   walk     one lane per query runs nearestQueryWalk (voxel_passes.h): an exact branch and bound on the sorted Morton codes of the set.  A node is a code prefix
//            with its range of the code array, its children are sub-ranges found by searches inside the range, a leaf's place is the vIndex.  A child is skipped
//            only when its box lies STRICTLY further than the best d2 so far or than the limit; the bound is seeded from the codes next to the query's own.
//   state    per lane and depth the range of the node there: dynamic LDS, ( levels - 1 ) rows of QB entries of 8 bytes, a column per lane (no bank conflict, no
//            private array); the children tried per depth are 4 bits each in two 64-bit registers.  0 bytes of scratch.
//   queries  either the caller's n x 3 int32, or made here from the codes of a second set and an offset: nothing of them travels to the host.
//   summary  (between) zero and beyond counts and the largest d2 within the limit: one atomic per wave; a second launch finds the lowest index that attains it.
//   transfer the 8 bytes of every voxel composed here, the changed ones counted, the voxels within the limit compacted into the list the attribute-only edit takes.
// No floating point, no lane waits on another, every loop is bounded (nearestQueryWalk).  The only atomics are the wave-reduced figures and the summary.
#include "launch.h"
#include "voxel_passes.h"

#define QB 64 // threads per workgroup of the walk: one wave, so that the LDS a group asks for is ( levels - 1 ) * 512 bytes
#define NB 256

namespace
{
thread_local NearestQueryStats g_queryStats;

enum // the slots of the device counters
{
	QS_VISITS = 0,
	QS_MOST = 1,
	QS_COMPARED = 2,
	QS_ZERO = 3,
	QS_BEYOND = 4,
	QS_MAXD2 = 5,
	QS_FARTHEST = 6, // preset to ~0
	QS_CHANGED = 7,
	QS_SLOTS = 8
};

// the ranges of one lane's path: rows of QB entries, this lane's column
struct LaneStack
{
	uint2* col;
	MVRT_DI void put( uint32_t d, uint32_t l, uint32_t h ) { col[d * QB] = make_uint2( l, h ); }
	MVRT_DI void get( uint32_t d, uint32_t& l, uint32_t& h ) const
	{
		const uint2 v = col[d * QB];
		l = v.x, h = v.y;
	}
};

// (waveSum, waveMax, waveMin and the Into forms, on unsigned long long here: voxel_passes.h)
typedef unsigned long long Count;

struct QueryOffset
{
	int32_t o[3];
};

// One lane per query.  query != null: the caller's points; else query i is voxel i of the set `from`, moved by -off.  Every output may be null; summary != 0
// adds the counts of mvrt_svo_nearest_between.  The lanes past n run no walk but take part in the wave reductions
__global__ void __launch_bounds__( QB ) kNearestQuery( const uint64_t* __restrict__ codes, const uint2* __restrict__ attrs, uint32_t nVoxels, uint32_t L,
														const int32_t* __restrict__ query, const uint64_t* __restrict__ from, QueryOffset off, uint32_t n, uint64_t maxDist2, int seed,
														int summary, uint64_t* __restrict__ dist2, uint32_t* __restrict__ nearest, uint2* __restrict__ attribs,
														unsigned long long* stats )
{
	extern __shared__ uint2 sRanges[]; // [L - 1][QB]; depth L - 1 never descends (its children are voxels) and is not stored
	const uint64_t i = (uint64_t)blockIdx.x * QB + threadIdx.x;
	NearestQueryAnswer r = { NEAREST_QUERY_NONE_D2, NEAREST_QUERY_NONE, 0u, 0u };
	const bool live = i < n;
	if( live )
	{
		int32_t qx, qy, qz;
		if( query ) qx = query[i * 3], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
		else nearestQueryOfVoxel( from[i], off.o, &qx, &qy, &qz );
		LaneStack stack = { sRanges + threadIdx.x };
		r = nearestQueryWalk( codes, nVoxels, L, qx, qy, qz, maxDist2, seed, stack );
		const bool found = r.near < nVoxels; // (NEAREST_QUERY_NONE is not below a count; checked before attrs is read)
		if( dist2 ) dist2[i] = r.d2;
		if( nearest ) nearest[i] = r.near;
		if( attribs ) attribs[i] = found ? nearestAttrib( attrs[r.near] ) : make_uint2( 0u, 0u );
	}
	const uint64_t visits = waveSum<Count>( r.visits ), most = waveMax<Count>( r.visits ), compared = waveSum<Count>( r.compared );
	const bool lane0 = waveLane0();
	if( lane0 )
	{
		atomicAdd( stats + QS_VISITS, (unsigned long long)visits );
		atomicAdd( stats + QS_COMPARED, (unsigned long long)compared );
		atomicMax( stats + QS_MOST, (unsigned long long)most );
	}
	if( !summary ) return;
	const bool within = live && r.d2 != NEAREST_QUERY_NONE_D2;
	// (three reductions, then the atomics: with waveAddInto the atomics stand between the reductions and the kernel's instructions change)
	const uint64_t zero = waveSum<Count>( within && r.d2 == 0ull ? 1ull : 0ull ), beyond = waveSum<Count>( live && !within ? 1ull : 0ull ), far = waveMax<Count>( within ? r.d2 : 0ull );
	if( lane0 )
	{
		if( zero ) atomicAdd( stats + QS_ZERO, (unsigned long long)zero );
		if( beyond ) atomicAdd( stats + QS_BEYOND, (unsigned long long)beyond );
		if( far ) atomicMax( stats + QS_MAXD2, (unsigned long long)far );
	}
}

// the second pass of the summary: the lowest query within the limit whose d2 is the largest (stats[QS_MAXD2], final: the walk's launch is done)
__global__ void __launch_bounds__( NB ) kQueryFarthest( const uint64_t* __restrict__ dist2, uint32_t n, unsigned long long* stats )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	const uint64_t want = stats[QS_MAXD2];
	const uint64_t mine = waveMin<Count>( i < n && dist2[i] == want ? i : ~0ull );
	if( waveLane0() && mine != ~0ull ) atomicMin( stats + QS_FARTHEST, (unsigned long long)mine );
}

// transfer: fresh[i] = the 8 bytes voxel i ends with, take[i] = 1 where it has a nearest voxel within the limit (it goes to the edit); the changed are counted
__global__ void __launch_bounds__( NB ) kTransferCompose( const uint2* __restrict__ own, const uint2* __restrict__ from, const uint32_t* __restrict__ nearest, uint32_t n, uint32_t flags,
														   uint2* __restrict__ fresh, uint32_t* __restrict__ take, unsigned long long* stats )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	uint64_t changed = 0ull;
	if( i < n )
	{
		const uint2 a = own[i];
		const bool within = nearest[i] != NEAREST_QUERY_NONE;
		const uint2 b = within ? nearestTransferAttrib( a, from[i], flags ) : a;
		fresh[i] = b;
		take[i] = within ? 1u : 0u;
		changed = a.x != b.x || a.y != b.y ? 1ull : 0ull;
	}
	waveAddInto<Count>( stats + QS_CHANGED, changed );
}
// the taken voxels in order: their cells and their bytes, the list of the edit.  offs = the n + 1 exclusive sums of take
__global__ void __launch_bounds__( NB ) kTransferList( const uint64_t* __restrict__ codes, const uint2* __restrict__ fresh, const uint32_t* __restrict__ take,
														const uint32_t* __restrict__ offs, uint32_t n, uint32_t* __restrict__ xyz, uint2* __restrict__ attribs )
{
	const uint64_t i = (uint64_t)blockIdx.x * NB + threadIdx.x;
	if( i >= n || !take[i] ) return;
	const uint64_t j = offs[i];
	mortonDecode( codes[i], xyz[j * 3], xyz[j * 3 + 1], xyz[j * 3 + 2] );
	attribs[j] = fresh[i];
}

// scan input.  (Not maskOffsets( take, n, 1u, ... ) of kernels_list.hip, which gives the same sums: without a scan instantiated in this file the compiler inlines
// __shfl_down into the three kernels above in another form, and their instructions are pinned by profiles/voxel_ops_refactor2_ab.txt)
struct TakeFlag
{
	const uint32_t* take;
	uint32_t n;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return i < n ? take[i] : 0u; }
};

int seedKnob() { return mvrtKnob( "MVRT_NEAREST_QUERY_SEED", 1 ) ? 1 : 0; } // (an experiment build can walk without the seed: tools/nearest_query_bench.py)

// (the counters of one call: Counters, voxel_passes.h, zeroed with QS_FARTHEST preset to ~0)
int launchWalk( const SurfaceSource& s, const int32_t* query, const uint64_t* from, const int32_t o[3], uint32_t n, uint64_t maxDist2, int summary, uint64_t* dist2, uint32_t* nearest,
				uint2* attribs, unsigned long long* stats, hipStream_t st )
{
	QueryOffset off = { { o ? o[0] : 0, o ? o[1] : 0, o ? o[2] : 0 } };
	const uint32_t lds = ( s.levels - 1u ) * QB * (uint32_t)sizeof( uint2 ); // 10 KB at 21 levels
	hipLaunchKernelGGL( kNearestQuery, dim3( divUp( n, QB ) ), dim3( QB ), lds, st, s.morton, s.attrs, s.nVoxels, s.levels, query, from, off, n, maxDist2, seedKnob(), summary, dist2,
						nearest, attribs, stats );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
// behind the last launch; waits for the stream
int readStats( const Counters& stats, uint32_t n, unsigned long long h[QS_SLOTS], hipStream_t st )
{
	if( stats.read( h, QS_SLOTS, st ) ) return 1;
	g_queryStats.queries = n;
	g_queryStats.visits = h[QS_VISITS];
	g_queryStats.mostVisits = h[QS_MOST];
	g_queryStats.compared = h[QS_COMPARED];
	return 0;
}
} // namespace

NearestQueryStats nearestQueryLastStats() { return g_queryStats; }

int nearestVoxels( const SurfaceSource& s, uint64_t n, const int32_t* queryDev, uint64_t maxDist2, uint64_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, hipStream_t st )
{
	g_queryStats = NearestQueryStats();
	if( n == 0 ) return 0; // no launch
	Counters stats;
	if( stats.init( QS_SLOTS, st, QS_FARTHEST ) ) return 1;
	// (the caller's arrays are written by this launch alone, behind the only allocation)
	if( launchWalk( s, queryDev, nullptr, nullptr, (uint32_t)n, maxDist2, 0, dist2Dev, nearestDev, (uint2*)attribsDev, stats.dev(), st ) ) return 1;
	unsigned long long h[QS_SLOTS];
	return readStats( stats, (uint32_t)n, h, st );
}

int nearestBetween( const SurfaceSource& a, const SurfaceSource& b, const int32_t o[3], uint64_t maxDist2, uint64_t capacity, uint64_t* dist2Dev, uint32_t* nearestDev,
					NearestBetweenCounts* counts, hipStream_t st )
{
	const char* who = "mvrt_svo_nearest_between";
	g_queryStats = NearestQueryStats();
	const uint32_t n = a.nVoxels;
	*counts = NearestBetweenCounts();
	counts->n = n;
	if( ( dist2Dev || nearestDev ) && capacity < n )
	{
		listingRefusal( who, "capacity", "voxels of a", capacity, n );
		return 1;
	}
	Counters stats;
	DevBuf own;
	if( stats.init( QS_SLOTS, st, QS_FARTHEST ) || ( !dist2Dev && own.alloc( (uint64_t)n * 8 ) ) ) return 1;
	uint64_t* d2 = dist2Dev ? dist2Dev : own.as<uint64_t>(); // (the second pass reads the distances: the summary call keeps them in scratch)
	if( launchWalk( b, nullptr, a.morton, o, n, maxDist2, 1, d2, nearestDev, nullptr, stats.dev(), st ) ) return 1;
	hipLaunchKernelGGL( kQueryFarthest, dim3( divUp( n, NB ) ), dim3( NB ), 0, st, d2, n, stats.dev() );
	MVRT_HIP( hipGetLastError() );
	unsigned long long h[QS_SLOTS];
	if( readStats( stats, n, h, st ) ) return 1;
	counts->nZero = h[QS_ZERO];
	counts->nBeyond = h[QS_BEYOND];
	counts->maxDist2 = h[QS_MAXD2];
	counts->farthest = h[QS_BEYOND] == n ? NEAREST_QUERY_NONE : (uint32_t)h[QS_FARTHEST]; // (every voxel beyond the limit: there is no farthest one)
	return 0;
}

int nearestTransferList( const SurfaceSource& dst, const SurfaceSource& src, const int32_t o[3], uint64_t maxDist2, uint32_t flags, DevBuf& xyz, DevBuf& attribs, uint64_t* nTaken,
						 uint64_t* nChanged, uint64_t* nBeyond, hipStream_t st )
{
	g_queryStats = NearestQueryStats();
	const uint32_t n = dst.nVoxels;
	const dim3 grid( divUp( n, NB ) ), block( NB );
	Counters stats;
	DevBuf near, from, fresh, take, offs;
	if( stats.init( QS_SLOTS, st, QS_FARTHEST ) || near.alloc( (uint64_t)n * 4 ) || from.alloc( (uint64_t)n * 8 ) || fresh.alloc( (uint64_t)n * 8 ) || take.alloc( (uint64_t)n * 4 ) ) return 1;
	if( launchWalk( src, nullptr, dst.morton, o, n, maxDist2, 1, nullptr, near.as<uint32_t>(), from.as<uint2>(), stats.dev(), st ) ) return 1;
	hipLaunchKernelGGL( kTransferCompose, grid, block, 0, st, dst.attrs, from.as<uint2>(), near.as<uint32_t>(), n, flags, fresh.as<uint2>(), take.as<uint32_t>(),
						stats.dev() );
	MVRT_HIP( hipGetLastError() );
	unsigned long long h[QS_SLOTS];
	if( readStats( stats, n, h, st ) ) return 1;
	near.release();
	from.release();
	*nChanged = h[QS_CHANGED];
	*nBeyond = h[QS_BEYOND];
	*nTaken = n - h[QS_BEYOND];
	if( *nChanged == 0 ) return 0; // no byte changes: no list
	if( exclusiveOffsetsOf<uint32_t>( TakeFlag{ take.as<uint32_t>(), n }, (uint64_t)n + 1, offs, nullptr, st ) ) return 1;
	if( xyz.alloc( *nTaken * 12 ) || attribs.alloc( *nTaken * 8 ) ) return 1;
	hipLaunchKernelGGL( kTransferList, grid, block, 0, st, dst.morton, fresh.as<uint2>(), take.as<uint32_t>(), offs.as<uint32_t>(), n, xyz.as<uint32_t>(), attribs.as<uint2>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
