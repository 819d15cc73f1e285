// exterior_host.hip -- gapLength and gapNodeOfCell of csrc/voxel_passes.h, the host-callable twins of what the exterior-masks kernel asks per neighbour cell
// (csrc/kernels_fill.hip), against brute force.  A program of its own: it makes no HIP call and needs no GPU.  Exit status 0 = every check
// held; each failure prints one line.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../massivevoxelraytracing_amd/csrc/voxel_passes.h"
#define HOST_CHECK_SEED 0x2545F4914F6CDD1Dull
#include "host_check.h"

static uint64_t keyOf( uint32_t L, uint64_t x, uint64_t y, uint64_t z ) { return ( ( ( z << L ) | y ) << L ) | x; }

// brute force: walk left and right from the cell along its row until a voxel or the end of the row.  -> the index of the voxel right of the cell when there is
// one on both sides (the gap's node), else 0
static uint32_t nodeSlow( const std::vector<uint64_t>& lin, uint32_t L, uint64_t key )
{
	const uint64_t R = 1ull << L, x = key & ( R - 1ull ), rowBase = key - x;
	bool left = false;
	for( uint64_t c = x; c-- > 0 && !left; ) left = std::binary_search( lin.begin(), lin.end(), rowBase + c );
	if( !left ) return 0u;
	for( uint64_t c = x + 1; c < R; c++ )
	{
		const auto it = std::lower_bound( lin.begin(), lin.end(), rowBase + c );
		if( it != lin.end() && *it == rowBase + c ) return (uint32_t)( it - lin.begin() );
	}
	return 0u;
}
static void checkCell( const char* name, const std::vector<uint64_t>& lin, uint32_t L, uint64_t key, int expectGap /* 1 yes, 0 no, -1 whatever brute force says */ )
{
	const uint32_t n = (uint32_t)lin.size();
	const uint32_t got = gapNodeOfCell( lin.data(), n, L, key ), want = nodeSlow( lin, L, key );
	CHECK( got == want, "%s: L = %u, key 0x%llx -> node %u, brute force says %u", name, L, (unsigned long long)key, got, want );
	if( expectGap >= 0 ) CHECK( ( got != 0u ) == ( expectGap == 1 ), "%s: key 0x%llx -> node %u", name, (unsigned long long)key, got );
	if( got )
	{
		// the node names gap got - 1: that gap exists and holds the cell
		const uint64_t len = gapLength( lin.data(), n, L, got - 1u );
		CHECK( len > 0 && lin[got - 1] < key && key <= lin[got - 1] + len, "%s: key 0x%llx is not a cell of gap %u (length %llu)", name, (unsigned long long)key, got - 1u,
			   (unsigned long long)len );
	}
}

// ---- the cases by hand ------------------------------------------------------------------------------------------------------------------------------------
static void testByHand()
{
	const uint32_t L = 3; // R = 8
	// rows (y, z): (2, 1) holds x = 1, 2, 5; (4, 1) holds x = 3, 6; (3, 1) holds nothing.  (1, 3) holds x = 0, 7
	std::vector<uint64_t> lin = { keyOf( L, 1, 2, 1 ), keyOf( L, 2, 2, 1 ), keyOf( L, 5, 2, 1 ), keyOf( L, 3, 4, 1 ), keyOf( L, 6, 4, 1 ), keyOf( L, 0, 1, 3 ), keyOf( L, 7, 1, 3 ) };
	std::sort( lin.begin(), lin.end() );
	checkCell( "before the first voxel of the list (j = 0)", lin, L, keyOf( L, 3, 0, 0 ), 0 );
	checkCell( "before the first voxel of the list, in its row (j = 0)", lin, L, keyOf( L, 0, 2, 1 ), 0 );
	checkCell( "behind the last voxel of the list (j = n)", lin, L, keyOf( L, 2, 5, 7 ), 0 );
	checkCell( "a voxel-free row between two occupied rows", lin, L, keyOf( L, 4, 3, 1 ), 0 );
	checkCell( "end run at x = 0", lin, L, keyOf( L, 0, 4, 1 ), 0 );
	checkCell( "end run behind the last voxel of a row, up to x = R - 1", lin, L, keyOf( L, 7, 4, 1 ), 0 );
	checkCell( "end run at x = R - 1, the next row starts at x = 0 of a later row", lin, L, keyOf( L, 7, 2, 1 ), 0 );
	checkCell( "a true gap, first cell", lin, L, keyOf( L, 3, 2, 1 ), 1 );
	checkCell( "a true gap, last cell", lin, L, keyOf( L, 4, 2, 1 ), 1 );
	checkCell( "a true gap of a row with border voxels", lin, L, keyOf( L, 4, 1, 3 ), 1 );
	checkCell( "lin[j - 1] in the previous row", lin, L, keyOf( L, 1, 4, 1 ), 0 ); // lin[j - 1] = (5, 2, 1), lin[j] = (3, 4, 1)
	CHECK( gapLength( lin.data(), (uint32_t)lin.size(), L, 0 ) == 0, "two voxels adjacent in x have no gap between them" );
	CHECK( gapLength( lin.data(), (uint32_t)lin.size(), L, 1 ) == 2, "x = 2 and x = 5: two cells" );
	CHECK( gapLength( lin.data(), (uint32_t)lin.size(), L, 2 ) == 0, "the last voxel of a row and the first of the next: no gap" );
	CHECK( gapLength( lin.data(), (uint32_t)lin.size(), L, 6 ) == 0, "the last voxel of the list" );
	CHECK( gapNodeOfCell( lin.data(), (uint32_t)lin.size(), L, keyOf( L, 3, 2, 1 ) ) == 2u, "the gap between voxels 1 and 2 is node 2" );
	// a list of one voxel, and the far corner of the largest grid (63-bit keys)
	const std::vector<uint64_t> one = { keyOf( L, 4, 4, 4 ) };
	for( uint64_t x = 0; x < 8; x++ )
		if( x != 4 ) checkCell( "one voxel", one, L, keyOf( L, x, 4, 4 ), 0 );
	const uint64_t T = ( 1ull << 21 ) - 1ull;
	const std::vector<uint64_t> far = { keyOf( 21, T - 4, T, T ), keyOf( 21, T, T, T ) };
	CHECK( gapNodeOfCell( far.data(), 2u, 21, keyOf( 21, T - 1, T, T ) ) == 1u && gapLength( far.data(), 2u, 21, 0 ) == 3, "a gap at the far corner of the 2^21 grid" );
	CHECK( gapNodeOfCell( far.data(), 2u, 21, keyOf( 21, T - 5, T, T ) ) == 0u && gapNodeOfCell( far.data(), 2u, 21, keyOf( 21, T - 1, T - 1, T ) ) == 0u, "beside that gap" );
}

// ---- random sorted key lists: every empty cell of the grid ---------------------------------------------------------------------------------------------------
static void testRandom()
{
	for( int round = 0; round < 60; round++ )
	{
		const uint32_t L = 2u + (uint32_t)( rnd() % 3u ); // R = 4, 8, 16
		const uint64_t cells = 1ull << ( 3u * L );
		const uint64_t density = rnd() % 100u; // per cent; 0 still leaves the one voxel below
		std::vector<uint64_t> lin;
		for( uint64_t c = 0; c < cells; c++ )
			if( rnd() % 100u < density ) lin.push_back( c );
		if( lin.empty() ) lin.push_back( rnd() % cells );
		for( uint64_t c = 0; c < cells; c++ )
			if( !std::binary_search( lin.begin(), lin.end(), c ) ) checkCell( "random", lin, L, c, -1 );
	}
}

int main()
{
	testByHand();
	testRandom();
	if( g_failures ) printf( "%d checks failed\n", g_failures );
	else printf( "exterior host checks ok\n" );
	return g_failures ? 1 : 0;
}
