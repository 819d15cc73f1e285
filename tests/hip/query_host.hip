// query_host.hip -- the nearest-voxel query run on the host: nearestQueryWalk of csrc/voxel_passes.h, the very function every lane of
// csrc/kernels_query.hip runs, against brute force over all voxels in __int128: the lexicographic minimum of ( squared distance, index in Morton order ).  The
// sets: random ones of 8^3 and 16^3 with queries inside the grid, on its border and up to 40 cells outside it, the single voxel, the two corners of the 2^21 grid
// queried from the far corner and from +-2^22, and the strict-tie case, which a local copy of the descent with the pruning rule flipped to >= gets wrong.  Every
// query is also asked with maxDist2 in { 0, d2 - 1, d2, d2 + 1 } and without the seed.  A program of its own: it makes no HIP call and needs no GPU.  Exit status
// 0 = every check held; each failure prints one line.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../massivevoxelraytracing_amd/csrc/voxel_passes.h"
#include "host_check.h"

struct Q
{
	int32_t x, y, z;
};
static uint64_t g_queries = 0, g_visits = 0, g_mostVisits = 0, g_deepest = 0;

// the definition: over ALL voxels, in an integer type twice as wide as the answer
static void brute( const std::vector<uint64_t>& codes, Q q, uint64_t* d2Out, uint32_t* nearOut )
{
	unsigned __int128 best = ~(unsigned __int128)0;
	uint32_t near = 0;
	for( size_t i = 0; i < codes.size(); i++ )
	{
		uint32_t x, y, z;
		mortonDecode( codes[i], x, y, z );
		const __int128 dx = (__int128)q.x - x, dy = (__int128)q.y - y, dz = (__int128)q.z - z;
		const unsigned __int128 d2 = (unsigned __int128)( dx * dx + dy * dy + dz * dz );
		if( d2 < best ) best = d2, near = (uint32_t)i; // (strict: the first, which is the lowest index, stays on a tie)
	}
	CHECK( best < ( (unsigned __int128)1 << 47 ), "d2 does not fit the 2^47 of the header" );
	*d2Out = (uint64_t)best;
	*nearOut = near;
}

static NearestQueryAnswer walk( const std::vector<uint64_t>& codes, uint32_t L, Q q, uint64_t maxDist2, int seed )
{
	NearestQueryHostStack stack;
	return nearestQueryWalk( codes.data(), codes.size(), L, q.x, q.y, q.z, maxDist2, seed, stack );
}

// one query: without a limit, with and without the seed, and at the four limits around its distance
static void checkQuery( const std::vector<uint64_t>& codes, uint32_t L, Q q, const char* name )
{
	uint64_t d2;
	uint32_t near;
	brute( codes, q, &d2, &near );
	g_queries++;
	g_deepest = std::max( g_deepest, d2 );
	for( int seed = 1; seed >= 0; seed-- )
	{
		const NearestQueryAnswer r = walk( codes, L, q, NEAREST_QUERY_NONE_D2, seed );
		CHECK( r.d2 == d2 && r.near == near, "%s seed %d: q (%d, %d, %d): ( %llu, %u ), brute force ( %llu, %u )", name, seed, q.x, q.y, q.z, (unsigned long long)r.d2, r.near,
			   (unsigned long long)d2, near );
		if( seed ) g_visits += r.visits, g_mostVisits = std::max<uint64_t>( g_mostVisits, r.visits );
	}
	const uint64_t limits[4] = { 0ull, d2 ? d2 - 1 : 0ull, d2, d2 + 1 };
	for( int k = 0; k < 4; k++ )
	{
		const NearestQueryAnswer r = walk( codes, L, q, limits[k], 1 );
		const bool within = d2 <= limits[k];
		CHECK( r.d2 == ( within ? d2 : NEAREST_QUERY_NONE_D2 ) && r.near == ( within ? near : NEAREST_QUERY_NONE ), "%s limit %llu: q (%d, %d, %d): ( %llu, %u ), d2 %llu near %u", name,
			   (unsigned long long)limits[k], q.x, q.y, q.z, (unsigned long long)r.d2, r.near, (unsigned long long)d2, near );
	}
}

static std::vector<uint64_t> sortedCodes( std::vector<uint64_t> c )
{
	std::sort( c.begin(), c.end() );
	c.erase( std::unique( c.begin(), c.end() ), c.end() );
	return c;
}

static void randomSets()
{
	for( int set = 0; set < 160; set++ )
	{
		const uint32_t L = ( set & 1 ) ? 4u : 3u, R = 1u << L;
		const uint32_t per1024 = set < 8 ? 1000u : 2u + (uint32_t)( rnd() % 300 ); // nearly full, then sparse to a third
		std::vector<uint64_t> c;
		for( uint32_t z = 0; z < R; z++ )
			for( uint32_t y = 0; y < R; y++ )
				for( uint32_t x = 0; x < R; x++ )
					if( rnd() % 1024 < per1024 ) c.push_back( mortonEncode( x, y, z ) );
		if( c.empty() ) c.push_back( mortonEncode( (uint32_t)( rnd() % R ), (uint32_t)( rnd() % R ), (uint32_t)( rnd() % R ) ) );
		const std::vector<uint64_t> codes = sortedCodes( c );
		const int32_t r = (int32_t)R;
		for( int k = 0; k < 48; k++ ) // inside the grid
			checkQuery( codes, L, Q{ (int32_t)( rnd() % R ), (int32_t)( rnd() % R ), (int32_t)( rnd() % R ) }, "inside" );
		for( int k = 0; k < 24; k++ ) // on its border: one coordinate at 0 or R - 1, and the cells just outside
		{
			Q q = { (int32_t)( rnd() % R ), (int32_t)( rnd() % R ), (int32_t)( rnd() % R ) };
			const int32_t edge[4] = { 0, r - 1, -1, r };
			( k % 3 == 0 ? q.x : k % 3 == 1 ? q.y : q.z ) = edge[( k / 3 ) & 3];
			checkQuery( codes, L, q, "border" );
		}
		for( int k = 0; k < 24; k++ ) // up to 40 cells outside it
			checkQuery( codes, L, Q{ (int32_t)( rnd() % ( R + 80 ) ) - 40, (int32_t)( rnd() % ( R + 80 ) ) - 40, (int32_t)( rnd() % ( R + 80 ) ) - 40 }, "outside" );
	}
}

static void singleVoxel()
{
	for( uint32_t L = 1; L <= 21; L += 4 )
	{
		const uint32_t last = ( 1u << L ) - 1u;
		const std::vector<uint64_t> codes = { mortonEncode( last, last / 2u, 0u ) };
		const Q qs[5] = { { (int32_t)last, (int32_t)( last / 2u ), 0 }, { 0, 0, 0 }, { -5, 7, (int32_t)last }, { -( 1 << 22 ), 1 << 22, -( 1 << 22 ) }, { 1 << 22, -( 1 << 22 ), 1 << 22 } };
		for( const Q& q : qs ) checkQuery( codes, L, q, "single voxel" );
	}
	// the 21-level path: one voxel at the far corner
	const uint32_t far = ( 1u << 21 ) - 1u;
	const std::vector<uint64_t> codes = { mortonEncode( far, far, far ) };
	checkQuery( codes, 21u, Q{ 0, 0, 0 }, "far corner" );
	checkQuery( codes, 21u, Q{ (int32_t)far, (int32_t)far, (int32_t)far }, "far corner" );
	checkQuery( codes, 21u, Q{ -( 1 << 22 ), -( 1 << 22 ), -( 1 << 22 ) }, "far corner" ); // the largest d2 there is: 3 ( 2^22 + 2^21 - 1 )^2, just below 2^47
	CHECK( g_deepest > ( 1ull << 46 ) && g_deepest < ( 1ull << 47 ), "a distance near 2^47 is among the cases: %llu", (unsigned long long)g_deepest );
}

static void twoCorners()
{
	const uint32_t far = ( 1u << 21 ) - 1u;
	const std::vector<uint64_t> codes = sortedCodes( { mortonEncode( 0u, 0u, 0u ), mortonEncode( far, far, far ) } );
	const int32_t f = (int32_t)far, m = 1 << 22;
	const Q qs[] = { { 0, 0, 0 }, { f, f, f }, { f, 0, 0 }, { 0, f, f }, { -m, -m, -m }, { m, m, m }, { m, -m, m }, { -m, m, -m }, { f / 2, f / 2, f / 2 }, { f / 2 + 1, f / 2 + 1, f / 2 + 1 },
					 { m, m, -m } };
	for( const Q& q : qs ) checkQuery( codes, 21u, q, "two corners" );
	uint64_t d2;
	uint32_t near;
	brute( codes, Q{ -m, -m, -m }, &d2, &near );
	CHECK( near == 0u && d2 == 3ull * ( 1ull << 44 ), "the corner at the origin is 2^22 off on every axis" );
	brute( codes, Q{ m, m, -m }, &d2, &near );
	CHECK( d2 > ( 1ull << 45 ), "a far query is among the cases: %llu", (unsigned long long)d2 );
}

// a local copy of the descent, recursive and without seed, run shortcut or child order; strict == false flips the pruning rule to >=
static void localWalk( const std::vector<uint64_t>& codes, uint32_t L, Q q, bool strict, uint32_t d, uint64_t lo, uint64_t hi, uint64_t prefix, uint32_t cx, uint32_t cy, uint32_t cz,
					   uint64_t* bestD2, uint32_t* bestV )
{
	const uint32_t s = L - d - 1u;
	const uint32_t oct = nearestOctant( q.x, q.y, q.z, cx, cy, cz, s );
	for( uint32_t k = 0; k < 8u; k++ )
	{
		const uint32_t c = nearestChildOrder( oct, k );
		uint64_t cLo, cHi;
		nearestChildRange( codes.data(), lo, hi, prefix, c, s, &cLo, &cHi );
		if( cLo == cHi ) continue;
		const uint32_t kx = cx | ( c & 1u ) << s, ky = cy | ( ( c >> 1 ) & 1u ) << s, kz = cz | ( c >> 2 ) << s;
		const uint64_t box = nearestBoxDist2( q.x, q.y, q.z, kx, ky, kz, s );
		if( strict ? box > *bestD2 : box >= *bestD2 ) continue;
		if( s == 0u )
		{
			if( nearestPairBelow( box, (uint32_t)cLo, *bestD2, *bestV ) ) *bestD2 = box, *bestV = (uint32_t)cLo;
			continue;
		}
		localWalk( codes, L, q, strict, d + 1u, cLo, cHi, prefix | (uint64_t)c << ( 3u * s ), kx, ky, kz, bestD2, bestV );
	}
}

// Two voxels at distance 1 of q = (8, 0, 0) in a 16^3 grid: A = (9, 0, 0) in q's own octant and B = (7, 0, 0), with the lower index, in the octant next to it, whose
// box lies at exactly the distance of A.  (7, 7, 7), the last code of B's octant, keeps B away from the seed.  `crowd` puts 27 far voxels into B's octant, so that
// the walk descends there instead of comparing a short run: the boxes on the way to B are all at distance 1 as well
static void strictTie( bool crowd )
{
	std::vector<uint64_t> c = { mortonEncode( 9u, 0u, 0u ), mortonEncode( 7u, 0u, 0u ), mortonEncode( 7u, 7u, 7u ) };
	if( crowd )
		for( uint32_t z = 5; z < 8; z++ )
			for( uint32_t y = 5; y < 8; y++ )
				for( uint32_t x = 0; x < 3; x++ ) c.push_back( mortonEncode( x, y, z ) );
	const std::vector<uint64_t> codes = sortedCodes( c );
	const Q q = { 8, 0, 0 };
	const uint32_t a = (uint32_t)( std::lower_bound( codes.begin(), codes.end(), mortonEncode( 9u, 0u, 0u ) ) - codes.begin() );
	uint64_t d2;
	uint32_t near;
	brute( codes, q, &d2, &near );
	CHECK( d2 == 1ull && near == 0u && codes[0] == mortonEncode( 7u, 0u, 0u ) && a == codes.size() - 1, "the case is what it says" );
	uint64_t seedD2 = NEAREST_QUERY_NONE_D2;
	uint32_t seedV = NEAREST_QUERY_NONE;
	nearestSeed( codes.data(), codes.size(), 4u, q.x, q.y, q.z, &seedD2, &seedV );
	CHECK( seedD2 == 1ull && seedV == a, "the seed finds A, not B: ( %llu, %u )", (unsigned long long)seedD2, seedV );
	CHECK( nearestBoxDist2( q.x, q.y, q.z, 0u, 0u, 0u, 3u ) == 1ull, "the box of B's octant is exactly as far as A" );
	checkQuery( codes, 4u, q, "strict tie" );
	for( int strict = 1; strict >= 0; strict-- )
	{
		uint64_t bd = NEAREST_QUERY_NONE_D2;
		uint32_t bv = NEAREST_QUERY_NONE;
		localWalk( codes, 4u, q, strict != 0, 0u, 0, codes.size(), 0ull, 0u, 0u, 0u, &bd, &bv );
		if( strict ) CHECK( bd == 1ull && bv == 0u, "the local copy with the strict rule finds B: ( %llu, %u )", (unsigned long long)bd, bv );
		else CHECK( bd == 1ull && bv == a, "the local copy with >= passes B's octant over and answers A: ( %llu, %u ) -- the case tells the two rules apart", (unsigned long long)bd, bv );
	}
}

static void helpers()
{
	for( uint32_t oct = 0; oct < 8u; oct++ )
	{
		uint32_t seen = 0u;
		for( uint32_t k = 0; k < 8u; k++ ) seen |= 1u << nearestChildOrder( oct, k );
		CHECK( seen == 0xFFu && nearestChildOrder( oct, 0u ) == oct && nearestChildOrder( oct, 7u ) == ( oct ^ 7u ), "the order visits every child once, the query's octant first" );
		CHECK( nearestChildOrder( oct, 3u ) == ( oct ^ 4u ) && nearestChildOrder( oct, 4u ) == ( oct ^ 3u ), "faces before edges" );
	}
	uint64_t w0 = 0, w1 = 0;
	for( uint32_t d = 0; d < 21u; d++ ) nearestTriedSet( w0, w1, d, ( d * 5u + 3u ) % 9u );
	for( uint32_t d = 0; d < 21u; d++ ) CHECK( nearestTriedGet( w0, w1, d ) == ( d * 5u + 3u ) % 9u, "depth %u keeps its count", d );
	CHECK( nearestPairBelow( 4, 9, 5, 1 ) && nearestPairBelow( 5, 1, 5, 2 ) && !nearestPairBelow( 5, 2, 5, 2 ) && !nearestPairBelow( 6, 0, 5, 2 ), "( d2, vIndex ) is compared as a pair" );
	CHECK( !nearestBoxSkipped( 5, 5, ~0ull ) && nearestBoxSkipped( 6, 5, ~0ull ) && nearestBoxSkipped( 3, 5, 2 ) && !nearestBoxSkipped( 2, 5, 2 ), "skipped only when strictly further" );
	const uint2 t = nearestTransferAttrib( make_uint2( 0x11223344u, 0x55667788u ), make_uint2( 0x0A0B0C0Du, 0x01020304u ), 1u );
	CHECK( t.x == 0xFF0B0C0Du && t.y == 0xFF667788u, "the colour word moves, the emission word stays, both alphas are 255" );
}

int main()
{
	helpers();
	randomSets();
	singleVoxel();
	twoCorners();
	strictTie( false );
	strictTie( true );
	printf( "queries %llu, visits per query %.2f, most %llu, deepest d2 %llu\n", (unsigned long long)g_queries, (double)g_visits / (double)g_queries, (unsigned long long)g_mostVisits,
			(unsigned long long)g_deepest );
	if( g_failures )
	{
		printf( "%d checks FAILED\n", g_failures );
		return 1;
	}
	printf( "query host checks ok\n" );
	return 0;
}
