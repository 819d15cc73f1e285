// kernels_resample.hip -- the voxel set of one octree resampled onto another grid under an affine map (mvrt_svo_resample_voxels / mvrt_svo_resample, mvrt.h;
// DESIGN.md 5.22).  The rule is nearest-neighbour resampling by inverse mapping, in integers: the centre of a destination cell is sent into the source grid by the
// fixed-point map of mvrt_cell_transform and the cell is a voxel when it lands in one (resamplePoint, voxel_passes.h).  The destination grid has up to 2^63 cells, so
// it is refined top-down instead of enumerated:
//
//   frontier  the Morton codes, ascending, of the destination nodes of one level that can still hold a result cell; level 0 is the whole grid, one node.
//   masks     8 lanes per node, one per child: the exact integer bounding box in source space of the child's sample points, clipped to the source grid
//             (resampleBox), and whether one of the at most 8 coarse source cells that cover the box holds a voxel (resampleBoxHoldsVoxel: one search of the sorted
//             codes per coarse cell).  At the last level the child is a cell and the test is the point rule itself.  A ballot gathers the 8 bits of a node.
//   expand    exclusive offsets over the popcounts of the masks, then the run expansion of voxel_passes.h: child r of a node is its r-th set bit.  Survivors are written
//             in the order of their parents, so every frontier and the result are in ascending Morton order without a sort.
//   emit      the expansion of the last level: per result cell the point rule once more, the search that returns the index of the source voxel, and code or
//             coordinates, attribute (colour and emission RGB, both alpha bytes 255) and source index; the emission flag is ORed once per wave.
// The pruning is conservative only: a node is dropped when no sample point of it can land in a voxel, so the result is the point rule's whatever the pruning keeps.
// Int64 arithmetic in plain C++, no floating point, no atomics but that OR.
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define RB 256 // threads per workgroup = items per workgroup of the run expansion

namespace
{
// One thread per child of the n nodes of `frontier`: gridDim.x = ceil( 8 n / RB ).  k = log2 of the child's edge in cells (0: the child is a cell).  The 8 lanes
// of a node are consecutive lanes of one wave
__global__ void __launch_bounds__( RB ) kResampleMasks( const uint64_t* __restrict__ frontier, uint64_t n, ResampleXf xf, uint32_t k, const uint64_t* __restrict__ codes,
														 uint32_t nSrc, uint32_t srcLevels, uint8_t* __restrict__ mask )
{
	const uint64_t i = (uint64_t)blockIdx.x * RB + threadIdx.x, node = i >> 3;
	bool keep = false;
	if( node < n )
	{
		uint32_t x, y, z;
		mortonDecode( frontier[node] << 3 | ( i & 7ull ), x, y, z );
		if( k == 0u )
		{
			int64_t s[3];
			keep = resamplePoint( xf, x, y, z, srcLevels, s ) && codePresentIn( codes, nSrc, mortonEncode( (uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[2] ) );
		}
		else
		{
			uint32_t lo[3], hi[3];
			keep = resampleBox( xf, x << k, y << k, z << k, k, srcLevels, lo, hi ) && resampleBoxHoldsVoxel( codes, nSrc, lo, hi );
		}
	}
	const uint64_t kept = __ballot( keep );
	if( node < n && ( i & 7ull ) == 0ull ) mask[node] = (uint8_t)( kept >> ( threadIdx.x & ( WAVE - 8 ) ) );
}
struct ChildCount // scan input: the surviving children of node i (item n: 0)
{
	const uint8_t* mask;
	uint32_t n;
	__host__ __device__ uint64_t operator()( uint32_t i ) const { return i < n ? (uint64_t)popcount8( mask[i] ) : 0ull; }
};

// offs: the n + 1 exclusive sums of the popcounts.  gridDim.x = ceil( n / RB ); a workgroup without survivors writes nothing
__global__ void __launch_bounds__( RB ) kResampleExpand( const uint64_t* __restrict__ frontier, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ offs, uint32_t n,
														  uint64_t* __restrict__ next )
{
	__shared__ uint32_t sOff[RB + 1];
	__shared__ uint64_t sCode[RB];
	__shared__ uint32_t sMask[RB];
	const uint64_t v = (uint64_t)blockIdx.x * RB + threadIdx.x;
	const uint64_t base = stageRunOffsets<RB>( offs, n, sOff ); // (relative offsets <= RB * 8)
	sCode[threadIdx.x] = v < n ? frontier[v] : 0ull;
	sMask[threadIdx.x] = v < n ? mask[v] : 0u;
	__syncthreads();
	const uint32_t total = sOff[RB];
	for( uint32_t j = threadIdx.x; j < total; j += RB )
	{
		const uint32_t lo = findRun( sOff, RB, j );
		next[base + j] = sCode[lo] << 3 | nthSetBit( sMask[lo], j - sOff[lo] );
	}
}
// The same expansion at the last level: a record is a result cell.  Every output may be null; attribsOut: two words per voxel, xyzOut three
__global__ void __launch_bounds__( RB ) kResampleEmit( const uint64_t* __restrict__ frontier, const uint8_t* __restrict__ mask, const uint64_t* __restrict__ offs, uint32_t n,
														ResampleXf xf, const uint64_t* __restrict__ codes, const uint2* __restrict__ attrs, uint32_t nSrc, uint32_t srcLevels,
														uint64_t* __restrict__ codesOut, uint32_t* __restrict__ attribsOut, uint32_t* __restrict__ xyzOut,
														uint32_t* __restrict__ sourceOut, uint32_t* __restrict__ hasEmission )
{
	__shared__ uint32_t sOff[RB + 1];
	__shared__ uint64_t sCode[RB];
	__shared__ uint32_t sMask[RB];
	const uint64_t v = (uint64_t)blockIdx.x * RB + threadIdx.x;
	const uint64_t base = stageRunOffsets<RB>( offs, n, sOff ); // (relative offsets <= RB * 8)
	sCode[threadIdx.x] = v < n ? frontier[v] : 0ull;
	sMask[threadIdx.x] = v < n ? mask[v] : 0u;
	__syncthreads();
	const uint32_t total = sOff[RB];
	uint32_t em = 0u;
	for( uint32_t j = threadIdx.x; j < total; j += RB )
	{
		const uint32_t lo = findRun( sOff, RB, j );
		const uint64_t c = sCode[lo] << 3 | nthSetBit( sMask[lo], j - sOff[lo] ), d = base + j;
		uint32_t x, y, z;
		int64_t s[3];
		mortonDecode( c, x, y, z );
		resamplePoint( xf, x, y, z, srcLevels, s ); // (in the grid and a voxel: the bit is set)
		uint64_t src = codeIndexIn( codes, nSrc, mortonEncode( (uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[2] ) );
		if( src >= nSrc ) src = nSrc - 1u; // (never: the mask kernel found it)
		const uint2 a = attrs[src];
		const uint2 at = make_uint2( a.x | 0xFF000000u, a.y | 0xFF000000u ); // the rule of MVRT_VOXEL_SET
		em |= at.y & 0xFFFFFFu;
		if( codesOut ) codesOut[d] = c;
		if( attribsOut )
		{
			attribsOut[d * 2] = at.x;
			attribsOut[d * 2 + 1] = at.y;
		}
		if( xyzOut )
		{
			xyzOut[d * 3] = x;
			xyzOut[d * 3 + 1] = y;
			xyzOut[d * 3 + 2] = z;
		}
		if( sourceOut ) sourceOut[d] = (uint32_t)src;
	}
	if( hasEmission && __ballot( em ) && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicOr( hasEmission, 1u );
}

thread_local ResampleStats g_lastStats;

// what the refinement leaves: the frontier of the last-but-one level with the masks and offsets of its children, the result cells (n of them)
struct Refined
{
	DevBuf frontier, mask, offs;
	uint32_t nNodes = 0;
	uint64_t n = 0;
};
// Has waited for the stream.  A frontier or a result of 2^32 - 1 entries or more is refused; `who` names the call
int refine( const char* who, const SurfaceSource& s, const ResampleXf& xf, uint32_t dstLevels, Refined* r, hipStream_t st )
{
	g_lastStats = ResampleStats();
	g_lastStats.levels = dstLevels;
	if( r->frontier.alloc( 8 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( r->frontier.p, 0, 8, st ) ); // level 0: the grid, code 0
	r->nNodes = 1;
	hipcub::CountingInputIterator<uint32_t> counting( 0u ); // (the one scan that keeps its hand-built iterator pair: profiles/voxel_ops_refactor2_ab.txt, section 5)
	for( uint32_t l = 1; l <= dstLevels; l++ ) // the level of the children
	{
		const uint32_t nNodes = r->nNodes;
		if( r->mask.alloc( nNodes ) ) return 1;
		hipLaunchKernelGGL( kResampleMasks, dim3( divUp( (uint64_t)nNodes * 8, RB ) ), dim3( RB ), 0, st, r->frontier.as<uint64_t>(), (uint64_t)nNodes, xf, dstLevels - l, s.morton,
							s.nVoxels, s.levels, r->mask.as<uint8_t>() );
		MVRT_HIP( hipGetLastError() );
		hipcub::TransformInputIterator<uint64_t, ChildCount, hipcub::CountingInputIterator<uint32_t>> counts( counting, ChildCount{ r->mask.as<uint8_t>(), nNodes } );
		uint64_t total = 0;
		if( exclusiveOffsets<uint64_t>( counts, (uint64_t)nNodes + 1, r->offs, &total, st ) ) return 1;
		g_lastStats.frontier[l] = total;
		r->n = l == dstLevels ? total : 0;
		if( total == 0 ) return 0; // nothing maps into a voxel
		if( total >= 0xFFFFFFFFull )
		{
			if( l == dstLevels ) mvrtSetError( "%s: the result would hold %llu voxels, beyond the 32-bit index range of the builder", who, (unsigned long long)total );
			else mvrtSetError( "%s: the frontier of level %u of the destination grid holds %llu nodes, beyond the 32-bit index range", who, l, (unsigned long long)total );
			return 1;
		}
		if( l == dstLevels ) return 0;
		DevBuf next;
		if( next.alloc( total * 8 ) ) return 1;
		hipLaunchKernelGGL( kResampleExpand, dim3( divUp( nNodes, RB ) ), dim3( RB ), 0, st, r->frontier.as<uint64_t>(), r->mask.as<uint8_t>(), r->offs.as<uint64_t>(), nNodes,
							next.as<uint64_t>() );
		MVRT_HIP( hipGetLastError() );
		MVRT_HIP( hipStreamSynchronize( st ) ); // (the old frontier is released here)
		r->frontier = std::move( next );
		r->nNodes = (uint32_t)total;
	}
	return 0;
}
// Not synchronised
int launchEmit( const Refined& r, const SurfaceSource& s, const ResampleXf& xf, uint64_t* codes, uint32_t* attribs, uint32_t* xyz, uint32_t* source, uint32_t* hasEmissionDev,
				hipStream_t st )
{
	hipLaunchKernelGGL( kResampleEmit, dim3( divUp( r.nNodes, RB ) ), dim3( RB ), 0, st, r.frontier.as<uint64_t>(), r.mask.as<uint8_t>(), r.offs.as<uint64_t>(), r.nNodes, xf, s.morton,
						s.attrs, s.nVoxels, s.levels, codes, attribs, xyz, source, hasEmissionDev );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
} // namespace

ResampleStats resampleLastStats() { return g_lastStats; }
bool resampleTransformValid( const int64_t m[9], const int64_t t[3] ) { return resampleTransformOk( m, t ); }
static ResampleXf makeXf( const int64_t m[9], const int64_t t[3] )
{
	ResampleXf xf;
	for( int k = 0; k < 9; k++ ) xf.m[k] = m[k];
	for( int i = 0; i < 3; i++ ) xf.t[i] = t[i];
	return xf;
}

int resampleVoxels( const SurfaceSource& s, const int64_t m[9], const int64_t t[3], uint32_t dstLevels, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* sourceDev, uint64_t* nOut,
					hipStream_t st )
{
	const ResampleXf xf = makeXf( m, t );
	Refined r;
	if( refine( "mvrt_svo_resample_voxels", s, xf, dstLevels, &r, st ) ) return 1;
	if( nOut ) *nOut = r.n;
	const int tail = listingTail( "mvrt_svo_resample_voxels", "capacity", "voxels", !xyzDev && !attribsDev && !sourceDev, capacity, r.n );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	if( launchEmit( r, s, xf, nullptr, attribsDev, xyzDev, sourceDev, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int resampleList( const char* who, const SurfaceSource& s, const int64_t m[9], const int64_t t[3], uint32_t dstLevels, SortedVoxels& out, hipStream_t st )
{
	const ResampleXf xf = makeXf( m, t );
	Refined r;
	if( refine( who, s, xf, dstLevels, &r, st ) ) return 1;
	out.n = (uint32_t)r.n;
	out.hasEmission = 0;
	if( r.n == 0 ) return 0;
	DevBuf flag;
	if( out.codes.alloc( r.n * 8 ) || out.attrs.alloc( r.n * 8 ) || flag.alloc( 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( flag.p, 0, 4, st ) );
	if( launchEmit( r, s, xf, out.codes.as<uint64_t>(), out.attrs.as<uint32_t>(), nullptr, nullptr, flag.as<uint32_t>(), st ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( &out.hasEmission, flag.p, 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
