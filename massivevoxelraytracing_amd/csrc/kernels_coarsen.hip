// kernels_coarsen.hip -- a coarser level of detail of the voxel set (mvrt_svo_coarse_voxels / mvrt_svo_coarsen, mvrt.h).  A streaming pass over
// the sorted codes and the Morton-ordered attributes a build leaves resident: code >> 3k is still ascending, so every coarse cell is one contiguous run of entries.
//
//   heads   entry i starts a cell when code >> 3k differs from its predecessor's (coarseHead, voxel_passes.h); rankHeads numbers the cells: cell = rank1[i] - 1.
//   reduce  one workgroup per CB = 1024 consecutive entries, four per thread.  Per cell the six channel sums and the count: first along the thread's own four
//           entries, then a segmented scan by head flags over the threads of the wave (shuffles), then over the four waves (LDS).  The entry that ends a cell's
//           stretch inside the workgroup holds the stretch's totals.  A cell that lies wholly inside the workgroup is written with plain stores; a cell that
//           straddles workgroups -- at most the first and the last stretch of a workgroup -- gets ONE atomic add per field from each workgroup it touches, into
//           accumulators zeroed beforehand.  Integer adds commute: the sums are exact and the same whatever the schedule.  No floating point anywhere.
//   finish  per cell keep = count >= minCount, the kept cells compacted by an exclusive scan of the keep flags (none for minCount = 1, which keeps all), then one
//           thread per cell emits code, attribute (coarseAttrib: six integer divisions, alpha 255), count, decoded coordinates and the emission flag.
//
// Inside a workgroup a sum is at most 255 * 1024 < 2^18 and a count at most 1024: three channels travel in one 64-bit word as 21-bit fields, so the scan moves two
// words and a count per step.  The accumulators across workgroups are 64-bit per channel (255 * (2^32 - 2) needs 40 bits); the count fits 32 (n < 2^32 - 1).
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define CT 256			 // threads per workgroup
#define CV 4			 // consecutive entries per thread: two 16-byte loads of codes, two of attributes, one of ranks
#define CB ( CT * CV ) // entries per workgroup of the reduce kernel

namespace
{
struct CoarseHeadFlag // scan input: 1 where entry i starts a coarse cell
{
	const uint64_t* codes;
	uint32_t shift;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return coarseHead( codes, i, shift ) ? 1u : 0u; }
};
struct CoarseKeptFlag // scan input: 1 where cell s is kept (item nSeg and beyond: 0)
{
	const uint32_t* counts;
	uint64_t minCount;
	uint32_t nSeg;
	__host__ __device__ uint32_t operator()( uint32_t s ) const { return s < nSeg && coarseKeep( counts[s], minCount ) ? 1u : 0u; }
};

// the sums of a stretch of at most CB entries: colour and emission as three 21-bit fields each (R | G << 21 | B << 42)
struct Part
{
	uint64_t col, emi;
	uint32_t cnt;
};
MVRT_DI uint64_t spread21( uint32_t rgba ) { return (uint64_t)( rgba & 0xFFu ) | (uint64_t)( ( rgba >> 8 ) & 0xFFu ) << 21 | (uint64_t)( ( rgba >> 16 ) & 0xFFu ) << 42; }
MVRT_DI void addTo( Part& a, const Part& b )
{
	a.col += b.col;
	a.emi += b.emi;
	a.cnt += b.cnt;
}

// rank1: the inclusive sums of the head flags (>= 1 for every entry).  sums: field f of cell s at sums[f * nSeg + s], zeroed, as counts; segCode[s] = the coarse code,
// written by the cell's head entry.  n >= 1, gridDim.x = ceil( n / CB ).
__global__ void __launch_bounds__( CT ) kCoarsenReduce( const uint64_t* __restrict__ codes, const uint2* __restrict__ attrs, const uint32_t* __restrict__ rank1, uint32_t n,
														 uint32_t shift, uint32_t nSeg, unsigned long long* __restrict__ sums, uint32_t* __restrict__ counts,
														 uint64_t* __restrict__ segCode )
{
	__shared__ uint64_t sCol[CT / WAVE], sEmi[CT / WAVE];
	__shared__ uint32_t sCnt[CT / WAVE], sFlag[CT / WAVE];
	const uint32_t lane = threadIdx.x & ( WAVE - 1 ), wave = threadIdx.x / WAVE;
	const uint64_t blockBase = (uint64_t)blockIdx.x * CB; // ( < n )
	const uint64_t i0 = blockBase + (uint64_t)threadIdx.x * CV;

	// ---- load: rank 0 = no such entry, which differs from every rank there is
	uint64_t c[CV];
	uint2 a[CV];
	uint32_t r[CV];
	if( i0 + CV <= n ) // (i0 is a multiple of 4: 32-byte aligned in all three arrays)
	{
		const ulonglong2 c01 = *(const ulonglong2*)( codes + i0 ), c23 = *(const ulonglong2*)( codes + i0 + 2 );
		const uint4 a01 = *(const uint4*)( attrs + i0 ), a23 = *(const uint4*)( attrs + i0 + 2 );
		const uint4 rr = *(const uint4*)( rank1 + i0 );
		c[0] = c01.x; c[1] = c01.y; c[2] = c23.x; c[3] = c23.y;
		a[0] = make_uint2( a01.x, a01.y ); a[1] = make_uint2( a01.z, a01.w ); a[2] = make_uint2( a23.x, a23.y ); a[3] = make_uint2( a23.z, a23.w );
		r[0] = rr.x; r[1] = rr.y; r[2] = rr.z; r[3] = rr.w;
	}
	else
	{
#pragma unroll
		for( uint32_t e = 0; e < CV; e++ )
		{
			const bool valid = i0 + e < n;
			c[e] = valid ? codes[i0 + e] : 0ull;
			a[e] = valid ? attrs[i0 + e] : make_uint2( 0u, 0u );
			r[e] = valid ? rank1[i0 + e] : 0u;
		}
	}
	const uint32_t rPrev = i0 > 0 && i0 <= n ? rank1[i0 - 1] : 0u;
	const uint32_t rNext = i0 + CV < n ? rank1[i0 + CV] : 0u;
	const uint32_t firstRank = rank1[blockBase];
	const bool blockStartsCell = blockBase == 0 || rank1[blockBase - 1] != firstRank;

	// ---- the thread's own entries: inc[e] = the sums from the last head at or before e, or from the thread's first entry
	bool head[CV];
	Part inc[CV];
	uint32_t anyHead = 0;
#pragma unroll
	for( uint32_t e = 0; e < CV; e++ )
	{
		head[e] = r[e] != ( e ? r[e - 1] : rPrev );
		Part v;
		v.col = spread21( a[e].x );
		v.emi = spread21( a[e].y );
		v.cnt = r[e] ? 1u : 0u;
		if( e && !head[e] ) addTo( v, inc[e - 1] );
		inc[e] = v;
		anyHead |= head[e] ? 1u : 0u;
	}

	// ---- segmented inclusive scan of the threads' last stretches over the wave, then the carry of the waves before
	Part run = inc[CV - 1];
	uint32_t flag = anyHead;
#pragma unroll
	for( uint32_t d = 1; d < WAVE; d <<= 1 )
	{
		Part o;
		o.col = __shfl_up( (unsigned long long)run.col, d, WAVE );
		o.emi = __shfl_up( (unsigned long long)run.emi, d, WAVE );
		o.cnt = __shfl_up( run.cnt, d, WAVE );
		const uint32_t of = __shfl_up( flag, d, WAVE );
		if( lane >= d )
		{
			if( !flag ) addTo( run, o );
			flag |= of;
		}
	}
	if( lane == WAVE - 1 )
	{
		sCol[wave] = run.col;
		sEmi[wave] = run.emi;
		sCnt[wave] = run.cnt;
		sFlag[wave] = flag;
	}
	Part carry; // what the entries before this thread add to its first stretch
	carry.col = __shfl_up( (unsigned long long)run.col, 1, WAVE );
	carry.emi = __shfl_up( (unsigned long long)run.emi, 1, WAVE );
	carry.cnt = __shfl_up( run.cnt, 1, WAVE );
	uint32_t carryFlag = __shfl_up( flag, 1, WAVE );
	if( lane == 0 )
	{
		carry.col = carry.emi = 0ull;
		carry.cnt = 0u;
		carryFlag = 0u;
	}
	__syncthreads();
	if( !carryFlag )
	{
		Part w = { 0ull, 0ull, 0u };
		for( uint32_t k = 0; k < wave; k++ )
		{
			Part o = { sCol[k], sEmi[k], sCnt[k] };
			if( !sFlag[k] ) addTo( o, w );
			w = o;
		}
		addTo( carry, w );
	}

	// ---- the entry that ends a cell's stretch in this workgroup writes the stretch
	const uint64_t m21 = ( 1ull << 21 ) - 1ull;
	bool headSeen = false;
#pragma unroll
	for( uint32_t e = 0; e < CV; e++ )
	{
		if( r[e] == 0u ) break; // past the end of the list
		headSeen = headSeen || head[e];
		const uint32_t s = r[e] - 1u; // ( < nSeg )
		if( head[e] ) segCode[s] = c[e] >> shift;
		const bool nextHead = ( e + 1 < CV ? r[e + 1] : rNext ) != r[e];
		const bool blockLast = i0 + e + 1 == blockBase + CB;
		if( !nextHead && !blockLast ) continue;
		Part t = inc[e];
		if( !headSeen ) addTo( t, carry );
		const unsigned long long f[6] = { t.col & m21, ( t.col >> 21 ) & m21, t.col >> 42, t.emi & m21, ( t.emi >> 21 ) & m21, t.emi >> 42 };
		const bool whole = nextHead && ( r[e] != firstRank || blockStartsCell ); // the cell begins and ends in this workgroup
		if( whole )
		{
#pragma unroll
			for( uint32_t k = 0; k < 6; k++ ) sums[(uint64_t)k * nSeg + s] = f[k];
			counts[s] = t.cnt;
		}
		else
		{
#pragma unroll
			for( uint32_t k = 0; k < 6; k++ ) atomicAdd( sums + (uint64_t)k * nSeg + s, f[k] );
			atomicAdd( counts + s, t.cnt );
		}
	}
}

// One thread per cell.  offs: the exclusive sums of the keep flags (nullptr: every cell is kept, cell s goes to place s).  Every output may be null; attribs: two
// words per cell
__global__ void __launch_bounds__( CT ) kCoarsenEmit( const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ counts, const uint64_t* __restrict__ segCode,
													   const uint32_t* __restrict__ offs, uint32_t nSeg, uint64_t minCount, uint64_t* __restrict__ codesOut,
													   uint32_t* __restrict__ attribsOut, uint32_t* __restrict__ countOut, uint32_t* __restrict__ xyzOut,
													   uint32_t* __restrict__ hasEmission )
{
	const uint64_t s = (uint64_t)blockIdx.x * CT + threadIdx.x;
	uint32_t em = 0;
	const uint32_t cnt = s < nSeg ? counts[s] : 0u;
	if( s < nSeg && coarseKeep( cnt, minCount ) )
	{
		const uint64_t d = offs ? offs[s] : s;
		uint64_t f[6];
#pragma unroll
		for( uint32_t k = 0; k < 6; k++ ) f[k] = sums[(uint64_t)k * nSeg + s];
		const uint2 at = coarseAttrib( f, cnt );
		const uint64_t code = segCode[s];
		if( codesOut ) codesOut[d] = code;
		if( attribsOut )
		{
			attribsOut[d * 2] = at.x;
			attribsOut[d * 2 + 1] = at.y;
		}
		if( countOut ) countOut[d] = cnt;
		if( xyzOut ) mortonDecode( code, xyzOut[d * 3], xyzOut[d * 3 + 1], xyzOut[d * 3 + 2] );
		em = at.y & 0xFFFFFFu;
	}
	if( hasEmission && __ballot( em ) && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicOr( hasEmission, 1u );
}

// what the reduce leaves: per cell the sums, the count and the coarse code, and the places of the kept cells (offs stays empty where every cell is kept)
struct Reduced
{
	DevBuf sums, counts, segCode, offs;
	uint32_t nSeg = 0, nKept = 0;
	bool reduced = false;
};
// countOnly: the number of kept cells is all that is wanted -- with minCount = 1 that is the number of cells and the reduce is left out.  Has waited for the stream.
int reduceCells( const uint64_t* morton, const uint2* attrs, uint32_t n, uint32_t levelsDown, uint64_t minCount, bool countOnly, Reduced* out, hipStream_t st )
{
	const uint32_t shift = 3u * levelsDown;
	DevBuf rank1;
	if( rankHeadsOf( CoarseHeadFlag{ morton, shift }, n, rank1, &out->nSeg, st ) ) return 1;
	const uint32_t nSeg = out->nSeg;
	out->nKept = nSeg;
	if( minCount == 1 && countOnly ) return 0;
	if( out->sums.alloc( (uint64_t)nSeg * 48 ) || out->counts.alloc( (uint64_t)nSeg * 4 ) || out->segCode.alloc( (uint64_t)nSeg * 8 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( out->sums.p, 0, (uint64_t)nSeg * 48, st ) );
	MVRT_HIP( hipMemsetAsync( out->counts.p, 0, (uint64_t)nSeg * 4, st ) );
	hipLaunchKernelGGL( kCoarsenReduce, dim3( divUp( n, CB ) ), dim3( CT ), 0, st, morton, attrs, rank1.as<uint32_t>(), n, shift, nSeg, out->sums.as<unsigned long long>(),
						out->counts.as<uint32_t>(), out->segCode.as<uint64_t>() );
	MVRT_HIP( hipGetLastError() );
	out->reduced = true;
	if( minCount == 1 )
	{
		MVRT_HIP( hipStreamSynchronize( st ) ); // (rank1 is released on return)
		return 0;
	}
	return exclusiveOffsetsOf<uint32_t>( CoarseKeptFlag{ out->counts.as<uint32_t>(), minCount, nSeg }, (uint64_t)nSeg + 1, out->offs, &out->nKept, st );
}
int launchEmit( const Reduced& r, uint64_t minCount, uint64_t* codes, uint32_t* attribs, uint32_t* count, uint32_t* xyz, uint32_t* hasEmission, hipStream_t st )
{
	hipLaunchKernelGGL( kCoarsenEmit, dim3( divUp( r.nSeg, CT ) ), dim3( CT ), 0, st, r.sums.as<unsigned long long>(), r.counts.as<uint32_t>(), r.segCode.as<uint64_t>(),
						r.offs.as<uint32_t>(), r.nSeg, minCount, codes, attribs, count, xyz, hasEmission );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
} // namespace

uint64_t coarseCellCapacity( int levelsDown ) { return coarseMaxCount( (uint32_t)levelsDown ); }

int coarseVoxels( const uint64_t* morton, const uint2* attrs, uint32_t n, int levelsDown, uint64_t minCount, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev,
				  uint32_t* countDev, uint64_t* nOut, hipStream_t st )
{
	const bool fill = xyzDev || attribsDev || countDev;
	Reduced r;
	if( reduceCells( morton, attrs, n, (uint32_t)levelsDown, minCount, !fill, &r, st ) ) return 1;
	if( nOut ) *nOut = r.nKept;
	const int tail = listingTail( "mvrt_svo_coarse_voxels", "capacity", "coarse voxels", !fill, capacity, r.nKept );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	if( launchEmit( r, minCount, nullptr, attribsDev, countDev, xyzDev, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int coarseCells( const uint64_t* morton, const uint2* attrs, uint32_t n, int levelsDown, DevBuf& codes, DevBuf& attribs, DevBuf& counts, uint32_t* nCells, hipStream_t st )
{
	Reduced r;
	if( reduceCells( morton, attrs, n, (uint32_t)levelsDown, 1, false, &r, st ) ) return 1;
	DevBuf a;
	if( a.alloc( (uint64_t)r.nSeg * 8 ) ) return 1;
	if( launchEmit( r, 1, nullptr, a.as<uint32_t>(), nullptr, nullptr, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the sums are released on return)
	codes = std::move( r.segCode ); // every cell is kept: the reduce's own arrays are the listing's, in its order
	counts = std::move( r.counts );
	attribs = std::move( a );
	*nCells = r.nSeg;
	return 0;
}

int coarseList( const uint64_t* morton, const uint2* attrs, uint32_t n, int levelsDown, uint64_t minCount, SortedVoxels& out, hipStream_t st )
{
	Reduced r;
	if( reduceCells( morton, attrs, n, (uint32_t)levelsDown, minCount, false, &r, st ) ) return 1;
	out.n = r.nKept;
	out.hasEmission = 0;
	if( r.nKept == 0 ) return 0;
	DevBuf flag;
	if( out.codes.alloc( (uint64_t)r.nKept * 8 ) || out.attrs.alloc( (uint64_t)r.nKept * 8 ) || flag.alloc( 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( flag.p, 0, 4, st ) );
	if( launchEmit( r, minCount, out.codes.as<uint64_t>(), out.attrs.as<uint32_t>(), nullptr, nullptr, flag.as<uint32_t>(), st ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( &out.hasEmission, flag.p, 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
