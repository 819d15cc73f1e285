// smooth_rule.h -- the arithmetic of mvrt_svo_surface_smooth (mvrt.h), host-callable so that a host program checks it exhaustively
// (tests/hip/smooth_host.hip): the rounded division, one relaxation step of one axis, the slot of a quad edge and the position of a displaced corner.
// Everything is int32: per axis |T| <= 256 + 6 * 128 + 6 * 128 = 1792 and |w| <= 256, so |w * T| < 2^19.
#pragma once
#include "mvrt_common.h"

#define SMOOTH_STEPS 256 // MVRT_SMOOTH_STEPS_PER_CELL

// rdiv( a, 256 * n ) for n in 2..6: sign( a ) * floor( ( 2|a| + 256 n ) / ( 512 n ) ), nearest with ties away from zero.  ( 2|a| + 256 n ) / ( 512 n ) =
// ( |a| + 128 n ) / ( 256 n ), and floor( floor( x / 256 ) / n ) = floor( x / ( 256 n ) ): a shift and a division by one of five constants
MVRT_HDI int32_t smoothRdiv( int32_t a, int32_t n )
{
	const uint32_t m = ( (uint32_t)( a < 0 ? -a : a ) + 128u * (uint32_t)n ) >> 8;
	uint32_t q;
	switch( n )
	{
	case 2: q = m / 2u; break;
	case 3: q = m / 3u; break;
	case 4: q = m / 4u; break;
	case 5: q = m / 5u; break;
	default: q = m / 6u; break;
	}
	return a < 0 ? -(int32_t)q : (int32_t)q;
}
// One axis of one vertex: d its displacement, sum = the sum of d_j over its n neighbours, unit = the sum of the neighbours' unit offsets on this axis (-1, 0
// or 1), w the weight of the iteration.  Returns the clamped d + delta; *clamped grows by 1 where d + delta lay outside [-limit, limit]
MVRT_HDI int32_t smoothStep( int32_t d, int32_t sum, int32_t unit, int32_t n, int32_t w, int32_t limit, uint32_t* clamped )
{
	const int32_t T = SMOOTH_STEPS * unit + sum - n * d;
	const int32_t v = d + smoothRdiv( w * T, n );
	if( v > limit )
	{
		( *clamped )++;
		return limit;
	}
	if( v < -limit )
	{
		( *clamped )++;
		return -limit;
	}
	return v;
}
// the slot (bit of the neighbour mask: 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z) of the step between two corner numbers of a voxel that differ on one axis
MVRT_HDI uint32_t smoothSlot( uint32_t cx0, uint32_t cy0, uint32_t cz0, uint32_t cx1, uint32_t cy1, uint32_t cz1 )
{
	return cx0 != cx1 ? ( cx1 > cx0 ? 1u : 0u ) : cy0 != cy1 ? ( cy1 > cy0 ? 3u : 2u ) : ( cz1 > cz0 ? 5u : 4u );
}
// the position on one axis of the corner c in [0, 2^21] displaced by d in [-128, 128]: q = 256 c + d <= 2^29 + 128, one conversion (rounded), an exact
// scaling, one multiply and one add, each rounded, never contracted.  d == 0 gives lower + (float)c * dps, the bits of mvrt_svo_surface_mesh
MVRT_HDI float smoothPosition( uint32_t c, int32_t d, float lower, float dps )
{
#pragma clang fp contract( off )
	const int32_t q = SMOOTH_STEPS * (int32_t)c + d;
	const float t = (float)q * 0.00390625f;
	const float p = t * dps;
	return lower + p;
}
