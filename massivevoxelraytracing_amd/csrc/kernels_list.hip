// kernels_list.hip -- the steps on sorted unique voxel lists that the voxel-set operators share (launch.h, "sorted voxel lists"): merge, gather of
// attributes, emission scan, compaction by a mask, the driver of a dilate / erode / close / open on a list, and the tail of a listing call.  Each step allocates its
// outputs itself and blocks unless it says otherwise.  No floating point, no atomics but the one-per-wave OR of the emission flag.
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define LB 256 // threads per workgroup

namespace
{
struct MaskFlag // scan input: 1 where entry i has ( removed = 1 ) or has not ( removed = 0 ) a mask bit set (item n: 0)
{
	const uint32_t* mask;
	uint32_t n, removed;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return i < n && ( mask[i] != 0u ) == ( removed != 0u ) ? 1u : 0u; }
};

// two sorted lists without a common code -> one: an entry's place is its own index plus the number of entries of the other list below it
__global__ void __launch_bounds__( LB ) kListMerge( const uint64_t* __restrict__ aCodes, const uint2* __restrict__ aAttrs, uint32_t nA, const uint64_t* __restrict__ bCodes,
													 const uint2* __restrict__ bAttrs, uint32_t nB, uint64_t* __restrict__ codes, uint2* __restrict__ attrs )
{
	const uint64_t i = (uint64_t)blockIdx.x * LB + threadIdx.x;
	if( i >= (uint64_t)nA + nB ) return;
	uint64_t c, d;
	uint2 a;
	if( i < nA )
	{
		c = aCodes[i];
		a = aAttrs[i];
		d = i + lowerBound( bCodes, 0, nB, c );
	}
	else
	{
		const uint64_t j = i - nA;
		c = bCodes[j];
		a = bAttrs[j];
		d = j + lowerBound( aCodes, 0, nA, c );
	}
	codes[d] = c;
	attrs[d] = a;
}

// offs: the exclusive sums of MaskFlag.  The flagged entries, in order: their code and attribute (a step) or their index (a listing); any output may be null
__global__ void __launch_bounds__( LB ) kListCompact( const uint64_t* __restrict__ codes, const uint2* __restrict__ attrs, const uint32_t* __restrict__ mask,
													   const uint32_t* __restrict__ offs, uint32_t n, uint32_t removed, uint64_t* __restrict__ codesOut,
													   uint2* __restrict__ attrsOut, uint32_t* __restrict__ vIndexOut )
{
	const uint64_t i = (uint64_t)blockIdx.x * LB + threadIdx.x;
	if( i >= n || ( mask[i] != 0u ) != ( removed != 0u ) ) return;
	const uint32_t d = offs[i];
	if( codesOut ) codesOut[d] = codes[i];
	if( attrsOut ) attrsOut[d] = attrs[i];
	if( vIndexOut ) vIndexOut[d] = (uint32_t)i;
}

// codes: a subset of srcCodes.  attrsOut[i] = the attribute the code has there
__global__ void __launch_bounds__( LB ) kListGatherAttrs( const uint64_t* __restrict__ codes, uint32_t n, const uint64_t* __restrict__ srcCodes,
														   const uint2* __restrict__ srcAttrs, uint32_t nSrc, uint2* __restrict__ attrsOut )
{
	const uint64_t i = (uint64_t)blockIdx.x * LB + threadIdx.x;
	if( i >= n ) return;
	const uint64_t j = lowerBound( srcCodes, 0, nSrc, codes[i] );
	attrsOut[i] = srcAttrs[j < nSrc ? j : nSrc - 1u];
}
__global__ void __launch_bounds__( LB ) kListAnyEmission( const uint2* __restrict__ attrs, uint32_t n, uint32_t* __restrict__ hasEmission )
{
	const uint64_t i = (uint64_t)blockIdx.x * LB + threadIdx.x;
	const uint32_t em = i < n ? attrs[i].y & 0xFFFFFFu : 0u;
	if( __ballot( em ) && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicOr( hasEmission, 1u );
}
} // namespace

int mergeLists( const uint64_t* aCodes, const uint2* aAttrs, uint32_t nA, const uint64_t* bCodes, const uint2* bAttrs, uint32_t nB, DevBuf& codes, DevBuf& attribs, hipStream_t st )
{
	const uint32_t nAll = nA + nB;
	if( codes.alloc( (uint64_t)nAll * 8 ) || attribs.alloc( (uint64_t)nAll * 8 ) ) return 1;
	hipLaunchKernelGGL( kListMerge, dim3( divUp( nAll, LB ) ), dim3( LB ), 0, st, aCodes, aAttrs, nA, bCodes, bAttrs, nB, codes.as<uint64_t>(), attribs.as<uint2>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) );
	return 0;
}
int gatherAttrs( const uint64_t* codes, uint32_t n, const uint64_t* srcCodes, const uint2* srcAttrs, uint32_t nSrc, DevBuf& attribs, hipStream_t st )
{
	if( attribs.alloc( (uint64_t)n * 8 ) ) return 1;
	hipLaunchKernelGGL( kListGatherAttrs, dim3( divUp( n, LB ) ), dim3( LB ), 0, st, codes, n, srcCodes, srcAttrs, nSrc, attribs.as<uint2>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipStreamSynchronize( st ) );
	return 0;
}
int anyEmission( const uint2* attrs, uint32_t n, uint32_t* hasEmission, hipStream_t st )
{
	DevBuf flag;
	if( flag.alloc( 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( flag.p, 0, 4, st ) );
	hipLaunchKernelGGL( kListAnyEmission, dim3( divUp( n, LB ) ), dim3( LB ), 0, st, attrs, n, flag.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	MVRT_HIP( hipMemcpyAsync( hasEmission, flag.p, 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	return 0;
}

int maskOffsets( const uint32_t* mask, uint32_t n, uint32_t removed, DevBuf& offs, uint32_t* count, hipStream_t st )
{
	return exclusiveOffsetsOf<uint32_t>( MaskFlag{ mask, n, removed }, (uint64_t)n + 1, offs, count, st );
}
int launchCompactMasked( const uint64_t* codes, const uint2* attrs, const uint32_t* mask, const uint32_t* offs, uint32_t n, uint32_t removed, uint64_t* codesOut, uint2* attrsOut,
						 uint32_t* vIndexOut, hipStream_t st )
{
	hipLaunchKernelGGL( kListCompact, dim3( divUp( n, LB ) ), dim3( LB ), 0, st, codes, attrs, mask, offs, n, removed, codesOut, attrsOut, vIndexOut );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
int compactUnmasked( const uint64_t* srcCodes, const uint2* srcAttrs, const uint32_t* mask, uint32_t n, bool scanEmission, SortedVoxels& out, hipStream_t st )
{
	DevBuf offs;
	out.hasEmission = 0;
	if( maskOffsets( mask, n, 0u, offs, &out.n, st ) ) return 1;
	if( out.n == n || out.n == 0 ) return 0;
	if( out.codes.alloc( (uint64_t)out.n * 8 ) || out.attrs.alloc( (uint64_t)out.n * 8 ) ) return 1;
	if( launchCompactMasked( srcCodes, srcAttrs, mask, offs.as<uint32_t>(), n, 0u, out.codes.as<uint64_t>(), out.attrs.as<uint2>(), nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) );
	offs.release();
	return scanEmission ? anyEmission( out.attrs.as<uint2>(), out.n, &out.hasEmission, st ) : 0;
}

int runListOperator( int op, const SurfaceSource& s, bool idleFirstHalfEnds, const ListHalf& dilate, const ListHalf& erode, SortedVoxels& out, hipStream_t st )
{
	VoxelList l( s.morton, s.attrs, s.nVoxels );
	out.n = s.nVoxels;
	out.hasEmission = 0;
	// the halves of a call: a dilation, an erosion or both, in the order of the operator
	const bool dilateFirst = op == MVRT_MORPH_OP_DILATE || op == MVRT_MORPH_OP_CLOSE;
	const int halves = op == MVRT_MORPH_OP_CLOSE || op == MVRT_MORPH_OP_OPEN ? 2 : 1;
	for( int h = 0; h < halves; h++ )
	{
		if( ( ( h == 0 ) == dilateFirst ? dilate : erode )( l ) ) return 1;
		if( idleFirstHalfEnds && h == 0 && l.n == s.nVoxels ) return 0;
	}
	out.n = l.n;
	// dilation grows, erosion shrinks, a closing holds the set and an opening lies in it: the same count is the same set, with the same bytes
	if( l.n == s.nVoxels ) return 0;
	if( op == MVRT_MORPH_OP_OPEN ) // a pure removal: the original bytes, not the ones the dilation half gave its cells
	{
		DevBuf original;
		if( gatherAttrs( l.codes, l.n, s.morton, s.attrs, s.nVoxels, original, st ) ) return 1;
		l.ownAttrs = std::move( original );
		l.attrs = l.ownAttrs.as<uint2>();
	}
	if( anyEmission( l.attrs, l.n, &out.hasEmission, st ) ) return 1;
	out.codes = std::move( l.ownCodes );
	out.attrs = std::move( l.ownAttrs );
	return 0;
}

int listingTail( const char* who, const char* capacityName, const char* things, bool sizing, uint64_t capacity, uint64_t n )
{
	if( sizing ) return LISTING_DONE;
	if( capacity < n )
	{
		listingRefusal( who, capacityName, things, capacity, n );
		return LISTING_REFUSED;
	}
	return n == 0 ? LISTING_DONE : LISTING_WRITE;
}
void listingRefusal( const char* who, const char* capacityName, const char* things, uint64_t capacity, uint64_t n )
{
	mvrtSetError( "%s: %s %llu is smaller than the %llu %s; nothing was written", who, capacityName, (unsigned long long)capacity, (unsigned long long)n, things );
}
