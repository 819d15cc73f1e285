// smooth_host.hip -- the arithmetic of mvrt_svo_surface_smooth (csrc/smooth_rule.h) without a GPU: the rounded division for every n in 2..6,
// every weight in [-256, 256] and every reachable T against floor arithmetic in int64 and against long double; the step (the sum, the clamp and its count) on a
// lattice of displacements, neighbour sums and limits; the slot of every quad edge against the corner offsets written out; the position at the corners 0, 1,
// 2^21 - 1 and 2^21 with d = +-128 against long double rounded at the same three places.  A program of its own: it makes no HIP call and needs no GPU.  Exit
// status 0 = every check held; each failure prints one line.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../massivevoxelraytracing_amd/csrc/smooth_rule.h"
#include "../../massivevoxelraytracing_amd/csrc/surface_weld.h"
#include "host_check.h"

#pragma clang fp contract( off ) // the plain-mesh position below is one multiply and one add

// floor( a / b ) for b > 0, written without a division of a negative number
static int64_t floorDiv( int64_t a, int64_t b ) { return a >= 0 ? a / b : -( ( -a + b - 1 ) / b ); }
// the rule as mvrt.h writes it: sign( a ) * floor( ( 2|a| + b ) / ( 2 b ) )
static int64_t rdivRule( int64_t a, int64_t b )
{
	const int64_t m = a < 0 ? -a : a;
	const int64_t q = floorDiv( 2 * m + b, 2 * b );
	return a < 0 ? -q : a > 0 ? q : 0;
}
#define MAX_T ( 256 + 6 * 128 + 6 * 128 ) // |256 u| + |sum of d_j| + |n d|

static void checkRdiv()
{
	int64_t largest = 0;
	for( int32_t n = 2; n <= 6; n++ )
		for( int32_t w = -256; w <= 256; w++ )
			for( int32_t T = -MAX_T; T <= MAX_T; T++ )
			{
				const int64_t a = (int64_t)w * T, b = 256 * (int64_t)n;
				const int64_t want = rdivRule( a, b );
				const long double x = fabsl( (long double)a ) / (long double)b + 0.5L; // a tie is k + 1/2 exactly; anything else is 1 / ( 2 b ) or more away from one
				const int64_t viaFloat = ( a < 0 ? -1 : 1 ) * (int64_t)floorl( x );
				const int32_t got = smoothRdiv( w * T, n );
				CHECK( got == want && want == viaFloat, "n %d w %d T %d: %d, rule %lld, long double %lld", n, w, T, got, (long long)want, (long long)viaFloat );
				CHECK( smoothRdiv( -( w * T ), n ) == -got, "n %d w %d T %d: not odd", n, w, T );
				largest = a > largest ? a : largest;
			}
	CHECK( largest < ( 1 << 20 ), "|w T| reaches %lld", (long long)largest );
}

static void checkStep()
{
	const int32_t ds[] = { -128, -127, -64, -1, 0, 1, 63, 127, 128 }, limits[] = { 0, 1, 64, 127, 128 };
	for( int32_t n = 2; n <= 6; n++ )
		for( int32_t w = -256; w <= 256; w++ )
			for( int32_t unit = -1; unit <= 1; unit++ )
				for( int32_t limit : limits )
					for( int32_t d0 : ds )
					{
						const int32_t d = d0 < -limit ? -limit : d0 > limit ? limit : d0; // a displacement the previous iteration can have left
						for( int32_t sum = -limit * n; sum <= limit * n; sum += ( limit * n ) / 16 + 1 )
						{
							const int64_t T = 256 * (int64_t)unit + sum - (int64_t)n * d;
							const int64_t v = d + rdivRule( (int64_t)w * T, 256 * (int64_t)n );
							const int64_t want = v > limit ? limit : v < -limit ? -limit : v;
							uint32_t clamped = 7;
							const int32_t got = smoothStep( d, sum, unit, n, w, limit, &clamped );
							CHECK( got == want && clamped == 7u + ( v != want ? 1u : 0u ), "n %d w %d unit %d limit %d d %d sum %d: %d (count %u), want %lld", n, w, unit, limit, d, sum, got,
								   clamped - 7u, (long long)want );
						}
					}
	// the figure of mvrt.h for a lone voxel: three neighbours, one of them a unit away on this axis, first iteration, plain weight
	uint32_t c = 0;
	CHECK( smoothStep( 0, 0, 1, 3, 256, 128, &c ) == 85 && smoothStep( 0, 0, -1, 3, 256, 128, &c ) == -85 && c == 0, "the first step of a cube corner" );
}

// the corner offsets and the corners of the six faces as mvrt.h lists them
static const int OFF[8][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 0, 1 }, { 0, 0, 1 }, { 0, 1, 0 }, { 1, 1, 0 }, { 1, 1, 1 }, { 0, 1, 1 } };
static const int FACE[6][4] = { { 3, 2, 1, 0 }, { 4, 5, 6, 7 }, { 0, 1, 5, 4 }, { 1, 2, 6, 5 }, { 2, 3, 7, 6 }, { 3, 0, 4, 7 } };

static void checkSlots()
{
	for( uint32_t d = 0; d < 6; d++ )
		for( uint32_t k = 0; k < 4; k++ )
		{
			const uint32_t c0 = faceCorner( d, k );
			CHECK( (int)c0 == FACE[d][k] && (int)cornerX( c0 ) == OFF[c0][0] && (int)cornerY( c0 ) == OFF[c0][1] && (int)cornerZ( c0 ) == OFF[c0][2], "face %u corner %u: %u", d, k, c0 );
			uint32_t seen = 0;
			for( uint32_t step = 1; step < 4; step += 2 )
			{
				const uint32_t c1 = faceCorner( d, ( k + step ) & 3u );
				const int u[3] = { OFF[c1][0] - OFF[c0][0], OFF[c1][1] - OFF[c0][1], OFF[c1][2] - OFF[c0][2] };
				const int axis = u[0] ? 0 : u[1] ? 1 : 2;
				CHECK( abs( u[0] ) + abs( u[1] ) + abs( u[2] ) == 1, "face %u corners %u and %u differ on more than one axis", d, k, ( k + step ) & 3u );
				const uint32_t want = 2u * (uint32_t)axis + ( u[axis] > 0 ? 1u : 0u );
				const uint32_t got = smoothSlot( cornerX( c0 ), cornerY( c0 ), cornerZ( c0 ), cornerX( c1 ), cornerY( c1 ), cornerZ( c1 ) );
				CHECK( got == want, "face %u corner %u step %u: slot %u, want %u", d, k, step, got, want );
				seen |= 1u << ( got >> 1 );
			}
			CHECK( __builtin_popcount( seen ) == 2, "face %u corner %u: both neighbours on one axis", d, k ); // the two edges of a quad corner span its plane
		}
}

static float positionRule( uint32_t c, int32_t d, float lower, float dps )
{
	const long double q = 256.0L * (long double)c + (long double)d;
	const float t = (float)( q / 256.0L ); // the conversion rounds once; the scaling by 2^-8 is exact before or behind it
	const float p = (float)( (long double)t * (long double)dps );
	return (float)( (long double)lower + (long double)p );
}
static uint32_t bitsOf( float f )
{
	uint32_t u;
	memcpy( &u, &f, 4 );
	return u;
}

static void checkPositions()
{
	const uint32_t corners[] = { 0u, 1u, ( 1u << 21 ) - 1u, 1u << 21, 12345u, ( 1u << 20 ) + 1u };
	const int32_t ds[] = { -128, -127, -1, 0, 1, 127, 128 };
	const float lowers[] = { -3.7f, 0.1f, 12.3f, 0.0f, -1048576.5f }, steps[] = { 0.1f, 1.0f, 0.0009765625f, 3.3e-5f, 7.25f };
	for( uint32_t c : corners )
		for( int32_t d : ds )
			for( float lower : lowers )
				for( float dps : steps )
				{
					const float got = smoothPosition( c, d, lower, dps ), want = positionRule( c, d, lower, dps );
					CHECK( bitsOf( got ) == bitsOf( want ), "corner %u d %d lower %g dps %g: %a, want %a", c, d, (double)lower, (double)dps, (double)got, (double)want );
					if( d == 0 )
					{
						const float plain = lower + (float)c * dps; // the position of mvrt_svo_surface_mesh
						CHECK( bitsOf( got ) == bitsOf( plain ), "corner %u lower %g dps %g: %a, the plain mesh has %a", c, (double)lower, (double)dps, (double)got, (double)plain );
					}
				}
	for( int k = 0; k < 200000; k++ ) // random corners and displacements, the same rule
	{
		const uint32_t c = (uint32_t)( rnd() % ( ( 1u << 21 ) + 1u ) );
		const int32_t d = (int32_t)( rnd() % 257u ) - 128;
		const float got = smoothPosition( c, d, -3.7f, 0.1f ), want = positionRule( c, d, -3.7f, 0.1f );
		CHECK( bitsOf( got ) == bitsOf( want ), "corner %u d %d: %a, want %a", c, d, (double)got, (double)want );
	}
}

int main()
{
	checkRdiv();
	checkStep();
	checkSlots();
	checkPositions();
	if( g_failures ) printf( "%d check(s) failed\n", g_failures );
	else printf( "smooth host checks ok\n" );
	return g_failures ? 1 : 0;
}
