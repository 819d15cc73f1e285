// kernels_walk.hip -- the voxels of an octree that keeps no Morton codes (an upload), recovered by walking it (mvrt_svo_walk_voxels / mvrt_svo_rebuild, mvrt.h).
//
// A root-to-voxel path, three bits per level with the root's slot highest, IS the voxel's Morton code, and the nVoxelsPSum values along it add up to the
// vIndex the traversal reports (device.hpp: voxelIndexFromPath).  The walk is breadth first, one level per pass, over a FRONTIER of paths: per entry the node
// word (embedded flavour: index | mask << 24 as the parent stores it; plain flavour: the index), the running nVoxelsPSum sum and the path prefix, three arrays.
//
//   count   children of entry i = popcount of its mask: the top byte of the word (embedded) or masks[node] (plain).  Not a kernel: the input iterator of
//   scan    a 64-bit exclusive sum (exclusiveOffsets, voxel_passes.h) over n + 1 items, the last one 0, so that offs[n] is the size of the next frontier.  It
//           goes to the host.
//   emit    the run expansion of voxel_passes.h: one workgroup per 256 parents, one thread per CHILD, its slot the k-th set bit of the parent's
//           mask; it reads children[c] and nVoxelsPSum[c] from the parent's 64-byte line.  Siblings are neighbouring lanes on one line; a wave writes 64
//           consecutive entries of each array.  The last level writes (code, vIndex) instead of a frontier entry.
//   gather  code -> xyz (x = bit 0 of each 3-bit group), attribs = attrs[vIndex] verbatim.  Also the read-back of a build's own list (mvrt_svo_read_voxels).
//
// Paths come out in ascending order: parents are in ascending prefix order and the children of one parent in ascending slot order.  A DAG is walked per PATH,
// shared nodes once per path that reaches them, so the count is the number of voxels, not of nodes.  Reachable nodes of mask 0 have no children: their path ends.
// What the walk relies on is the upload contract (mvrt.h rules 2-4, checked on the host before an upload is accepted) or the builder: child words below
// numberOfNodes, voxels in the last level only, sums below numberOfVoxels.  A word that names no node is still read as a node of mask 0, and an index past the
// attributes as zero attributes: nothing here reads out of bounds whatever the nodes hold.
#include "launch.h"
#include "voxel_passes.h"

#define WB 256 // threads per workgroup, and parents per workgroup of the emit kernel

namespace
{
// own mask of the node a frontier word names.  masks == nullptr: embedded flavour, the word carries it
MVRT_HDI uint32_t wordMask( uint32_t w, const uint8_t* __restrict__ masks, uint32_t nNodes )
{
	if( masks ) return w < nNodes ? (uint32_t)masks[w] : 0u;
	return ( w & 0xFFFFFFu ) < nNodes ? w >> 24 : 0u;
}
struct ChildCount // scan input: children of frontier entry i; item n is the 0 behind the last entry
{
	const uint32_t* word;
	const uint8_t* masks;
	uint32_t nNodes;
	uint64_t n;
	__host__ __device__ uint64_t operator()( uint64_t i ) const { return i < n ? popcount8( wordMask( word[i], masks, nNodes ) ) : 0ull; }
};

// One workgroup per WB parents, the run expansion of voxel_passes.h: offs = nParents + 1 exclusive offsets, the records are children (at most 8 * WB a group), a
// parent's children the set bits of its mask.  LAST: the children are voxels -> cPrefix = the Morton code, cSum = the vIndex, cWord is not written.
template <bool EMB, bool LAST>
__global__ void __launch_bounds__( WB ) kWalkEmit( const Node64* __restrict__ nodes, const uint8_t* __restrict__ masks, const uint32_t* __restrict__ psumCold, uint32_t nNodes,
												   const uint32_t* __restrict__ pWord, const uint32_t* __restrict__ pSum, const uint64_t* __restrict__ pPrefix,
												   const uint64_t* __restrict__ offs, uint64_t nParents, uint32_t* __restrict__ cWord, uint32_t* __restrict__ cSum,
												   uint64_t* __restrict__ cPrefix )
{
	__shared__ uint32_t sOff[WB + 1];
	__shared__ uint32_t sWord[WB];
	__shared__ uint32_t sSum[WB];
	__shared__ uint64_t sPrefix[WB];
	__shared__ uint8_t sMask[WB];
	const uint64_t p = (uint64_t)blockIdx.x * WB + threadIdx.x;
	const bool in = p < nParents;
	const uint64_t base = stageRunOffsets<WB>( offs, nParents, sOff );
	const uint32_t w = in ? pWord[p] : 0u;
	sWord[threadIdx.x] = w;
	sMask[threadIdx.x] = in ? (uint8_t)wordMask( w, EMB ? nullptr : masks, nNodes ) : (uint8_t)0;
	sSum[threadIdx.x] = in ? pSum[p] : 0u;
	sPrefix[threadIdx.x] = in ? pPrefix[p] : 0ull;
	__syncthreads();
	const uint32_t total = sOff[WB];
	for( uint32_t j = threadIdx.x; j < total; j += WB )
	{
		const uint32_t lo = findRun( sOff, WB, j );
		const uint32_t c = nthSetBit( sMask[lo], j - sOff[lo] );
		const uint32_t node = EMB ? sWord[lo] & 0xFFFFFFu : sWord[lo]; // (a parent with children has a mask, so it is below nNodes: wordMask)
		const Node64& line = nodes[node];
		const uint32_t ps = EMB ? line.psum[c] : psumCold[(uint64_t)node * 8u + c];
		const uint64_t out = base + j;
		if( !LAST ) cWord[out] = line.children[c];
		cSum[out] = sSum[lo] + ps;
		cPrefix[out] = ( sPrefix[lo] << 3 ) | c;
	}
}

// The read-back of voxels, walked (launchWalkGather) or kept by a build (svoReadVoxels).  vIndex == nullptr: the codes are the sorted list of a build and entry i
// is voxel i.  Any output may be null.
__global__ void __launch_bounds__( WB ) kWalkGather( const uint64_t* __restrict__ codes, const uint32_t* __restrict__ vIndex, const uint2* __restrict__ attrs, uint32_t nVoxels,
													 uint64_t n, uint32_t* __restrict__ xyz, uint32_t* __restrict__ vIndexOut, uint32_t* __restrict__ attribs )
{
	for( uint64_t i = (uint64_t)blockIdx.x * WB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WB )
	{
		const uint32_t v = vIndex ? vIndex[i] : (uint32_t)i;
		if( xyz ) mortonDecode( codes[i], xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2] );
		if( vIndexOut ) vIndexOut[i] = v;
		if( attribs )
		{
			const uint2 a = v < nVoxels ? attrs[v] : make_uint2( 0u, 0u );
			attribs[i * 2] = a.x;
			attribs[i * 2 + 1] = a.y;
		}
	}
}

struct Frontier
{
	DevBuf word, sum, prefix;
	int alloc( uint64_t n ) { return word.alloc( n * 4 ) || sum.alloc( n * 4 ) || prefix.alloc( n * 8 ); }
};

template <bool EMB, bool LAST>
void launchEmit( const WalkSource& s, const Frontier& par, const uint64_t* offs, uint64_t nParents, uint32_t* cWord, uint32_t* cSum, uint64_t* cPrefix, hipStream_t st )
{
	hipLaunchKernelGGL( ( kWalkEmit<EMB, LAST> ), dim3( divUp( nParents, WB ) ), dim3( WB ), 0, st, s.nodes, s.masks, s.psumCold, s.nNodes, par.word.as<uint32_t>(),
						par.sum.as<uint32_t>(), par.prefix.as<uint64_t>(), offs, nParents, cWord, cSum, cPrefix );
}
} // namespace

int launchWalkGather( const uint64_t* codes, const uint32_t* vIndex, const uint2* attrs, uint32_t nVoxels, uint64_t n, uint32_t* xyz, uint32_t* vIndexOut, uint32_t* attribs,
					  hipStream_t st )
{
	if( n == 0 ) return 0;
	const uint64_t blocks = ( n + WB - 1 ) / WB;
	hipLaunchKernelGGL( kWalkGather, dim3( (uint32_t)( blocks > 65536 ? 65536 : blocks ) ), dim3( WB ), 0, st, codes, vIndex, attrs, nVoxels, n, xyz, vIndexOut, attribs );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
// mvrt_svo_read_voxels: the sorted list of a build, entry i = voxel i, on the builder's grid of 1 to 4096 groups.  Waits for the stream.
int svoReadVoxels( const uint64_t* morton, const uint2* attrs, uint32_t n, uint32_t* xyz, uint32_t* attribs, hipStream_t st )
{
	const uint64_t blocks = ( (uint64_t)n + WB - 1 ) / WB;
	hipLaunchKernelGGL( kWalkGather, dim3( (uint32_t)( blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks ) ), dim3( WB ), 0, st, morton, nullptr, attrs, n, n, xyz, nullptr, attribs );
	MVRT_HIP( hipStreamSynchronize( st ) );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// One host synchronisation that waits per level (the size of the next frontier), one more behind the last emit.  Every buffer is a DevBuf of this call: a failed
// allocation returns an error and leaks nothing.  The buffers alternate between two sets, so what a level allocates over was last read two levels earlier, by
// launches the previous level's synchronisation has already seen finish.
int walkPaths( const WalkSource& s, bool fill, uint64_t fillLimit, WalkResult* out, hipStream_t st )
{
	out->n = 0;
	out->filled = 0;
	if( s.levels == 0 || s.nNodes == 0 ) return 0;
	Frontier fr[2];
	DevBuf offs[2];
	struct SyncOnExit // declared behind the buffers, so it runs before they go: an error return never frees what a launch in flight still reads
	{
		hipStream_t st;
		~SyncOnExit() { (void)hipStreamSynchronize( st ); }
	} syncOnExit{ st };
	if( fr[0].alloc( 1 ) ) return 1;
	const uint32_t rootWord = ( s.nNodes - 1u ) | ( s.embedded ? s.rootMask << 24 : 0u );
	MVRT_HIP( hipMemcpyAsync( fr[0].word.p, &rootWord, 4, hipMemcpyHostToDevice, st ) ); // (rootWord outlives the first synchronisation below)
	MVRT_HIP( hipMemsetAsync( fr[0].sum.p, 0, 4, st ) );
	MVRT_HIP( hipMemsetAsync( fr[0].prefix.p, 0, 8, st ) );
	uint64_t n = 1;
	for( uint32_t d = 0; d < s.levels; d++ )
	{
		const Frontier& par = fr[d & 1u];
		Frontier& kid = fr[( d + 1u ) & 1u];
		DevBuf& off = offs[d & 1u];
		const bool last = d + 1u == s.levels;
		uint64_t total = 0;
		if( exclusiveOffsetsOf<uint64_t, uint64_t>( ChildCount{ par.word.as<uint32_t>(), s.embedded ? nullptr : s.masks, s.nNodes, n }, n + 1, off, &total, st ) ) return 1;
		if( last ) out->n = total;
		if( total == 0 ) return 0; // every path ended in a node of mask 0 (the empty octree: the root)
		if( last && ( !fill || total > fillLimit ) ) return 0;
		if( ( n + WB - 1 ) / WB > 0x7FFFFFFFull )
		{
			mvrtSetError( "octree walk: a frontier of %llu paths is beyond one launch", (unsigned long long)n );
			return 1;
		}
		if( last )
		{
			if( out->codes.alloc( total * 8 ) || out->vIndex.alloc( total * 4 ) ) return 1;
			if( s.embedded ) launchEmit<true, true>( s, par, off.as<uint64_t>(), n, nullptr, out->vIndex.as<uint32_t>(), out->codes.as<uint64_t>(), st );
			else launchEmit<false, true>( s, par, off.as<uint64_t>(), n, nullptr, out->vIndex.as<uint32_t>(), out->codes.as<uint64_t>(), st );
			MVRT_HIP( hipGetLastError() );
			MVRT_HIP( hipStreamSynchronize( st ) ); // (the frontier and the offsets are released on return)
			out->filled = 1;
			return 0;
		}
		if( kid.alloc( total ) ) return 1;
		if( s.embedded ) launchEmit<true, false>( s, par, off.as<uint64_t>(), n, kid.word.as<uint32_t>(), kid.sum.as<uint32_t>(), kid.prefix.as<uint64_t>(), st );
		else launchEmit<false, false>( s, par, off.as<uint64_t>(), n, kid.word.as<uint32_t>(), kid.sum.as<uint32_t>(), kid.prefix.as<uint64_t>(), st );
		MVRT_HIP( hipGetLastError() );
		n = total;
	}
	return 0;
}
