// kernels_combine.hip -- union, intersection, difference and symmetric difference of two voxel sets, the second moved by an integer cell offset
// (mvrt_svo_combine_voxels / mvrt_svo_combine, mvrt.h).  Both operands are sorted unique lists of codes with their attributes; so is the result.
//
//   translate  skipped when the offset is zero and b's grid is not larger than a's: b's codes are then B' as they are.  Otherwise one thread per entry of b
//              decodes, adds, clips and encodes (combineTranslate, voxel_passes.h: 64-bit sums, nothing wraps), the survivors are compacted behind an exclusive
//              scan and sorted by the 3 * levels( a ) bits of their code (sortPairsInto), the value being the entry of b the attribute comes from.
//   classify   one thread per entry of A and one per entry of B': its lower bound in the other list (the partner position, one search of the whole list), whether
//              the code stands there (the overlap) and whether the entry survives the operator.  A voxel of the overlap survives as the entry of A, never as that of B'.
//   emit       exclusive scans of the survive flags of both lists; a survivor goes to its own offset plus the offset of the other list at its partner position
//              (the rule of kListMerge with holes).  One scatter writes code or coordinates, attribute and source byte, and ORs the emission flag once per wave.
// No floating point, no atomics but that OR.
#include "launch.h"
#include "voxel_passes.h"

#define WAVE 64
#define KB 256 // threads per workgroup

namespace
{
struct Offset3
{
	int32_t v[3];
};
// keys[i] = the code of entry i of b in a's grid, ~0 where the offset moves it out (a code has 63 bits at most)
__global__ void __launch_bounds__( KB ) kCombineTranslate( const uint64_t* __restrict__ bCodes, uint32_t nB, Offset3 o, uint32_t levels, uint64_t* __restrict__ keys )
{
	const uint64_t i = (uint64_t)blockIdx.x * KB + threadIdx.x;
	if( i >= nB ) return;
	uint64_t c = 0ull;
	keys[i] = combineTranslate( bCodes[i], o.v, levels, &c ) ? c : ~0ull;
}
struct InGrid // scan input: 1 where entry i of b stays in the grid (item n: 0)
{
	const uint64_t* keys;
	uint32_t n;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return i < n && keys[i] != ~0ull ? 1u : 0u; }
};
// offs: the exclusive sums of InGrid.  The survivors in b's order: code and entry
__global__ void __launch_bounds__( KB ) kCombineCompact( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ offs, uint32_t nB, uint64_t* __restrict__ keysOut,
														  uint32_t* __restrict__ idxOut )
{
	const uint64_t i = (uint64_t)blockIdx.x * KB + threadIdx.x;
	if( i >= nB ) return;
	const uint64_t c = keys[i];
	if( c == ~0ull ) return;
	const uint32_t d = offs[i];
	keysOut[d] = c;
	idxOut[d] = (uint32_t)i;
}

// state of an entry: bit 0 = its code is in the other list too, bit 1 = it is part of the result
#define ST_BOTH 1u
#define ST_LIVES 2u
// One thread per entry of `mine`: partner = lowerBound of its code in `other` (0 .. nOther), state as above with livesAlone / livesBoth = what the operator decides
// for an entry that is in this list only / in both.  Every lane searches the whole list.  The form that bounded the search once per workgroup (combineWindow,
// voxel_passes.h: thread 0 finds the window of the group's 256 ascending codes, the lanes search inside it) was built and measured: a third slower on both bench
// scenes, the lanes waiting behind two dependent searches of one thread, so it is not here.
__global__ void __launch_bounds__( KB ) kCombineClassify( const uint64_t* __restrict__ mine, uint32_t nMine, const uint64_t* __restrict__ other, uint32_t nOther, uint32_t livesAlone,
														   uint32_t livesBoth, uint32_t* __restrict__ partner, uint8_t* __restrict__ state )
{
	const uint64_t i = (uint64_t)blockIdx.x * KB + threadIdx.x;
	if( i >= nMine ) return;
	const uint64_t c = mine[i];
	const uint64_t p = lowerBound( other, 0, nOther, c );
	const bool both = p < nOther && other[p] == c;
	partner[i] = (uint32_t)p;
	state[i] = (uint8_t)( ( both ? ST_BOTH : 0u ) | ( ( both ? livesBoth : livesAlone ) ? ST_LIVES : 0u ) );
}
struct Lives // scan input: 1 where entry i is part of the result (item n: 0)
{
	const uint8_t* state;
	uint32_t n;
	__host__ __device__ uint32_t operator()( uint32_t i ) const { return i < n ? ( state[i] >> 1 ) & 1u : 0u; }
};

struct CombineSide // one operand, classified: n entries, partner / state per entry, offs = the n + 1 exclusive sums of Lives
{
	const uint64_t* codes;
	const uint2* attrs;
	const uint32_t* idx; // entry i carries attrs[idx[i]] (nullptr: attrs[i])
	const uint32_t* partner;
	const uint8_t* state;
	const uint32_t* offs;
	uint32_t n;
};
MVRT_DI uint2 attribOfB( const CombineSide& b, uint64_t j ) // the rule of MVRT_VOXEL_SET: colour and emission RGB, both alpha bytes 255
{
	const uint2 a = b.attrs[b.idx ? b.idx[j] : j];
	return make_uint2( a.x | 0xFF000000u, a.y | 0xFF000000u );
}
// One thread per entry of A, then of B'.  Every output may be null; attribsOut: two words per voxel, xyzOut three
__global__ void __launch_bounds__( KB ) kCombineEmit( CombineSide a, CombineSide b, uint32_t attribB, uint64_t* __restrict__ codesOut, uint32_t* __restrict__ attribsOut,
													   uint32_t* __restrict__ xyzOut, uint8_t* __restrict__ sourceOut, uint32_t* __restrict__ hasEmission )
{
	const uint64_t i = (uint64_t)blockIdx.x * KB + threadIdx.x;
	bool lives = false;
	uint64_t c = 0ull, d = 0ull;
	uint2 at = make_uint2( 0u, 0u );
	uint32_t src = 0u;
	if( i < a.n )
	{
		const uint32_t st = a.state[i];
		if( st & ST_LIVES )
		{
			const uint32_t p = a.partner[i];
			lives = true;
			c = a.codes[i];
			d = (uint64_t)a.offs[i] + b.offs[p];
			src = ( st & ST_BOTH ) ? 3u : 1u;
			at = ( st & ST_BOTH ) && attribB ? attribOfB( b, p ) : a.attrs[i];
		}
	}
	else if( i - a.n < b.n )
	{
		const uint64_t j = i - a.n;
		if( b.state[j] & ST_LIVES )
		{
			lives = true;
			c = b.codes[j];
			d = (uint64_t)b.offs[j] + a.offs[b.partner[j]];
			src = 2u;
			at = attribOfB( b, j );
		}
	}
	if( lives )
	{
		if( codesOut ) codesOut[d] = c;
		if( attribsOut )
		{
			attribsOut[d * 2] = at.x;
			attribsOut[d * 2 + 1] = at.y;
		}
		if( xyzOut ) mortonDecode( c, xyzOut[d * 3], xyzOut[d * 3 + 1], xyzOut[d * 3 + 2] );
		if( sourceOut ) sourceOut[d] = (uint8_t)src;
	}
	if( hasEmission && __ballot( lives && ( at.y & 0xFFFFFFu ) ) && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicOr( hasEmission, 1u );
}

// partner, state and offs of one list against the other (all allocated here); *nLives = its entries in the result.  Has waited for the stream
struct Classified
{
	DevBuf partner, state, offs;
	uint32_t nLives = 0;
};
int classify( const uint64_t* mine, uint32_t nMine, const uint64_t* other, uint32_t nOther, bool livesAlone, bool livesBoth, Classified* out, hipStream_t st )
{
	if( out->partner.alloc( (uint64_t)nMine * 4 ) || out->state.alloc( nMine ) ) return 1;
	if( nMine )
	{
		hipLaunchKernelGGL( kCombineClassify, dim3( divUp( nMine, KB ) ), dim3( KB ), 0, st, mine, nMine, other, nOther, livesAlone ? 1u : 0u, livesBoth ? 1u : 0u,
							out->partner.as<uint32_t>(), out->state.as<uint8_t>() );
		MVRT_HIP( hipGetLastError() );
	}
	return exclusiveOffsetsOf<uint32_t>( Lives{ out->state.as<uint8_t>(), nMine }, (uint64_t)nMine + 1, out->offs, &out->nLives, st );
}

// both operands classified under an operator: what the listing and the in-place call emit from
struct Plan
{
	DevBuf bKeys, bIdx; // B' where it had to be made
	Classified ca, cb;
	CombineSide a, b;
	uint64_t n = 0, nOverlap = 0, nClipped = 0;
};
// B' = b's codes as they are, or translated, clipped, compacted and sorted.  Has waited for the stream
int translate( const SurfaceSource& a, const SurfaceSource& b, const int32_t o[3], Plan* p, hipStream_t st )
{
	p->b.attrs = b.attrs;
	if( o[0] == 0 && o[1] == 0 && o[2] == 0 && b.levels <= a.levels )
	{
		p->b.codes = b.morton;
		p->b.idx = nullptr;
		p->b.n = b.nVoxels;
		return 0;
	}
	DevBuf keys, offs, keysA, idxA;
	if( keys.alloc( (uint64_t)b.nVoxels * 8 ) ) return 1;
	Offset3 off;
	off.v[0] = o[0];
	off.v[1] = o[1];
	off.v[2] = o[2];
	const dim3 grid( divUp( b.nVoxels, KB ) ), block( KB );
	hipLaunchKernelGGL( kCombineTranslate, grid, block, 0, st, b.morton, b.nVoxels, off, a.levels, keys.as<uint64_t>() );
	MVRT_HIP( hipGetLastError() );
	uint32_t nIn = 0;
	if( exclusiveOffsetsOf<uint32_t>( InGrid{ keys.as<uint64_t>(), b.nVoxels }, (uint64_t)b.nVoxels + 1, offs, &nIn, st ) ) return 1;
	p->nClipped = b.nVoxels - nIn;
	p->b.n = nIn;
	p->b.codes = nullptr;
	p->b.idx = nullptr;
	if( nIn == 0 ) return 0;
	if( keysA.alloc( (uint64_t)nIn * 8 ) || idxA.alloc( (uint64_t)nIn * 4 ) ) return 1;
	hipLaunchKernelGGL( kCombineCompact, grid, block, 0, st, keys.as<uint64_t>(), offs.as<uint32_t>(), b.nVoxels, keysA.as<uint64_t>(), idxA.as<uint32_t>() );
	MVRT_HIP( hipGetLastError() );
	if( sortPairsInto( keysA, idxA, nIn, (int)( 3u * a.levels ), p->bKeys, p->bIdx, st ) ) return 1;
	p->b.codes = p->bKeys.as<uint64_t>();
	p->b.idx = p->bIdx.as<uint32_t>();
	return 0;
}
int makePlan( const SurfaceSource& a, const SurfaceSource& b, int op, const int32_t o[3], Plan* p, hipStream_t st )
{
	if( translate( a, b, o, p, st ) ) return 1;
	p->a.codes = a.morton;
	p->a.attrs = a.attrs;
	p->a.idx = nullptr;
	p->a.n = a.nVoxels;
	// an entry of A alone lives unless the operator is the intersection, the overlap lives (as the entry of A) under union and intersection; an entry of B'
	// alone lives under union and symmetric difference
	const bool aAlone = op != MVRT_COMBINE_OP_INTERSECTION, both = op == MVRT_COMBINE_OP_UNION || op == MVRT_COMBINE_OP_INTERSECTION;
	const bool bAlone = op == MVRT_COMBINE_OP_UNION || op == MVRT_COMBINE_OP_XOR;
	if( classify( p->a.codes, p->a.n, p->b.codes, p->b.n, aAlone, both, &p->ca, st ) ) return 1;
	if( classify( p->b.codes, p->b.n, p->a.codes, p->a.n, bAlone, false, &p->cb, st ) ) return 1;
	p->a.partner = p->ca.partner.as<uint32_t>();
	p->a.state = p->ca.state.as<uint8_t>();
	p->a.offs = p->ca.offs.as<uint32_t>();
	p->b.partner = p->cb.partner.as<uint32_t>();
	p->b.state = p->cb.state.as<uint8_t>();
	p->b.offs = p->cb.offs.as<uint32_t>();
	p->n = (uint64_t)p->ca.nLives + p->cb.nLives;
	// the overlap from the counts alone: what lives of A is A without the overlap (difference, xor), the overlap (intersection) or all of A (union)
	const uint64_t nA = p->a.n, nB = p->b.n;
	switch( op )
	{
	case MVRT_COMBINE_OP_UNION: p->nOverlap = nB - p->cb.nLives; break;
	case MVRT_COMBINE_OP_INTERSECTION: p->nOverlap = p->ca.nLives; break;
	default: p->nOverlap = nA - p->ca.nLives; break;
	}
	return 0;
}
// Not synchronised
int launchEmit( const Plan& p, uint32_t attribB, uint64_t* codes, uint32_t* attribs, uint32_t* xyz, uint8_t* source, uint32_t* hasEmissionDev, hipStream_t st )
{
	hipLaunchKernelGGL( kCombineEmit, dim3( divUp( (uint64_t)p.a.n + p.b.n, KB ) ), dim3( KB ), 0, st, p.a, p.b, attribB, codes, attribs, xyz, source, hasEmissionDev );
	MVRT_HIP( hipGetLastError() );
	return 0;
}
} // namespace

int combineVoxels( const SurfaceSource& a, const SurfaceSource& b, int op, const int32_t o[3], uint32_t flags, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev,
				   uint8_t* sourceDev, uint64_t* nOut, uint64_t* nOverlapOut, uint64_t* nClippedOut, hipStream_t st )
{
	Plan p;
	if( makePlan( a, b, op, o, &p, st ) ) return 1;
	if( nOut ) *nOut = p.n;
	if( nOverlapOut ) *nOverlapOut = p.nOverlap;
	if( nClippedOut ) *nClippedOut = p.nClipped;
	const int tail = listingTail( "mvrt_svo_combine_voxels", "capacity", "voxels", !xyzDev && !attribsDev && !sourceDev, capacity, p.n );
	if( tail != LISTING_WRITE ) return tail;
	// (the caller's arrays are written by this launch alone, behind every allocation and check)
	if( launchEmit( p, flags & MVRT_COMBINE_FLAG_ATTRIB_B, nullptr, attribsDev, xyzDev, sourceDev, nullptr, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}

int combineList( const char* who, const SurfaceSource& a, const SurfaceSource& b, int op, const int32_t o[3], uint32_t flags, CombineCounts* c, hipStream_t st )
{
	Plan p;
	if( makePlan( a, b, op, o, &p, st ) ) return 1;
	SortedVoxels& out = c->list;
	out.n = a.nVoxels;
	out.hasEmission = 0;
	c->nAdded = p.cb.nLives;
	c->nRemoved = a.nVoxels - p.ca.nLives;
	c->nOverlap = p.nOverlap;
	c->nClipped = p.nClipped;
	const bool keepsOverlap = op == MVRT_COMBINE_OP_UNION || op == MVRT_COMBINE_OP_INTERSECTION;
	c->recolours = ( flags & MVRT_COMBINE_FLAG_ATTRIB_B ) && keepsOverlap && p.nOverlap > 0 ? 1u : 0u;
	if( c->nAdded == 0 && c->nRemoved == 0 && !c->recolours ) return 0; // nothing changes
	if( p.n == 0 )
	{
		mvrtSetError( "%s: the operation would leave no voxel (it removes all %u)", who, a.nVoxels );
		return 1;
	}
	if( p.n >= 0xFFFFFFFFull )
	{
		mvrtSetError( "%s: the result would hold %llu voxels, beyond the 32-bit index range of the builder", who, (unsigned long long)p.n );
		return 1;
	}
	out.n = (uint32_t)p.n;
	DevBuf flag;
	const bool structural = c->nAdded != 0 || c->nRemoved != 0; // else the codes are a's own: the attributes alone
	if( ( structural && out.codes.alloc( p.n * 8 ) ) || out.attrs.alloc( p.n * 8 ) || flag.alloc( 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( flag.p, 0, 4, st ) );
	if( launchEmit( p, c->recolours, structural ? out.codes.as<uint64_t>() : nullptr, out.attrs.as<uint32_t>(), nullptr, nullptr, flag.as<uint32_t>(), st ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( &out.hasEmission, flag.p, 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
