// combine_host.hip -- the helpers of csrc/voxel_passes.h that the kernels of csrc/kernels_combine.hip are built on (combineTranslate, combineWindow,
// codeIndexInRange), against brute force: the translation on grids of gridRes 2 and 4 for every offset in [-R, R]^3 and at the borders of the 2^21
// grid, where nothing may be folded back, and the windowed search against codeIndexIn on random sorted lists.  A program of its own: it makes no HIP call and needs
// no GPU.  Exit status 0 = every check held; each failure prints one line.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../massivevoxelraytracing_amd/csrc/voxel_passes.h"
#include "host_check.h"

// one cell, one offset: inside exactly when every moved coordinate lies in [0, R), and then the code of the moved cell
static void checkOne( long long x, long long y, long long z, const int32_t o[3], uint32_t levels )
{
	const long long R = 1ll << levels, nx = x + o[0], ny = y + o[1], nz = z + o[2];
	const bool inside = nx >= 0 && nx < R && ny >= 0 && ny < R && nz >= 0 && nz < R;
	uint64_t got = 0x5A5A5A5A5A5A5A5Aull;
	const bool ok = combineTranslate( encodeSlow( (uint64_t)x, (uint64_t)y, (uint64_t)z ), o, levels, &got );
	CHECK( ok == inside, "(%lld, %lld, %lld) + (%d, %d, %d), levels %u: inside %d, got %d", x, y, z, o[0], o[1], o[2], levels, (int)inside, (int)ok );
	if( ok && inside )
		CHECK( got == encodeSlow( (uint64_t)nx, (uint64_t)ny, (uint64_t)nz ), "(%lld, %lld, %lld) + (%d, %d, %d), levels %u: code %llx", x, y, z, o[0], o[1], o[2], levels,
			   (unsigned long long)got );
	if( !ok ) CHECK( got == 0x5A5A5A5A5A5A5A5Aull, "a clipped cell wrote a code" );
}
// every cell of a source grid of gridRes 2, 4 and 8 into target grids of gridRes 2 and 4, for every offset in [-R, R]^3 (R of the target) and a few beyond
static void checkTranslateSmall()
{
	for( uint32_t levels = 1; levels <= 2; levels++ )
		for( int srcRes = 2; srcRes <= 8; srcRes *= 2 )
		{
			const int R = 1 << levels;
			for( int x = 0; x < srcRes; x++ )
				for( int y = 0; y < srcRes; y++ )
					for( int z = 0; z < srcRes; z++ )
						for( int ox = -R - 1; ox <= R + 1; ox++ )
							for( int oy = -R - 1; oy <= R + 1; oy++ )
								for( int oz = -R - 1; oz <= R + 1; oz++ )
								{
									const int32_t o[3] = { ox, oy, oz };
									checkOne( x, y, z, o, levels );
								}
		}
}
// the borders of the largest grid: coordinates 0 and 2^21 - 1, offsets +-1 and +-2^21, on every axis and in combination; and the same cells into smaller grids
static void checkTranslateBorders()
{
	const long long top = ( 1ll << 21 ) - 1;
	const long long coords[4] = { 0, 1, top - 1, top };
	const int32_t offs[7] = { 0, 1, -1, 1 << 21, -( 1 << 21 ), ( 1 << 21 ) - 1, -( ( 1 << 21 ) - 1 ) };
	const uint32_t levelsOfTarget[3] = { 21, 20, 1 };
	for( uint32_t levels : levelsOfTarget )
		for( long long x : coords )
			for( long long y : coords )
				for( long long z : coords )
					for( int32_t ox : offs )
						for( int32_t oy : offs )
							for( int32_t oz : offs )
							{
								const int32_t o[3] = { ox, oy, oz };
								checkOne( x, y, z, o, levels );
							}
	// spelled out: nothing is folded back
	uint64_t c = 0;
	const int32_t plus[3] = { 1, 0, 0 }, minus[3] = { 0, -1, 0 }, far[3] = { 1 << 21, 0, 0 }, back[3] = { 0, 0, -( 1 << 21 ) };
	CHECK( !combineTranslate( encodeSlow( top, 5, 9 ), plus, 21, &c ), "2^21 - 1 + 1 stays outside" );
	CHECK( !combineTranslate( encodeSlow( 5, 0, 9 ), minus, 21, &c ), "0 - 1 stays outside" );
	CHECK( !combineTranslate( encodeSlow( 0, 5, 9 ), far, 21, &c ), "0 + 2^21 = R stays outside" );
	CHECK( !combineTranslate( encodeSlow( 5, 9, top ), back, 21, &c ), "2^21 - 1 - 2^21 = -1 stays outside" );
	CHECK( combineTranslate( encodeSlow( top - 1, 5, 9 ), plus, 21, &c ) && c == encodeSlow( top, 5, 9 ), "2^21 - 2 + 1 is the last cell" );
	CHECK( combineTranslate( encodeSlow( 5, 1, 9 ), minus, 21, &c ) && c == encodeSlow( 5, 0, 9 ), "1 - 1 is the first cell" );
}

// a group of ascending codes [g0, g1) of `mine` against `other`: the window holds every partner, and the search inside it is the search in the whole list
static void checkGroup( const std::vector<uint64_t>& mine, size_t g0, size_t g1, const std::vector<uint64_t>& other, const char* what )
{
	const uint64_t n = other.size();
	const uint64_t* codes = other.data(); // (never read where n == 0)
	uint64_t lo = ~0ull, hi = ~0ull;
	combineWindow( codes, n, mine[g0], mine[g1 - 1], &lo, &hi );
	CHECK( lo <= hi && hi <= n, "%s: window [%llu, %llu) of %llu", what, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)n );
	if( lo > hi || hi > n ) return;
	for( uint64_t k = 0; k < lo; k++ ) CHECK( other[k] < mine[g0], "%s: entry %llu before the window is not below the group", what, (unsigned long long)k );
	for( uint64_t k = hi; k < n; k++ ) CHECK( other[k] >= mine[g1 - 1], "%s: entry %llu behind the window is below the group's last", what, (unsigned long long)k );
	for( size_t i = g0; i < g1; i++ )
	{
		const uint64_t want = codeIndexIn( codes, n, mine[i] ), got = codeIndexInRange( codes, n, lo, hi, mine[i] );
		CHECK( got == want, "%s: code %llx -> %llu, codeIndexIn says %llu (window [%llu, %llu) of %llu)", what, (unsigned long long)mine[i], (unsigned long long)got,
			   (unsigned long long)want, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)n );
		CHECK( lowerBound( codes, lo, hi, mine[i] ) == lowerBound( codes, 0, n, mine[i] ), "%s: code %llx: the lower bound in the window differs", what, (unsigned long long)mine[i] );
	}
}
static std::vector<uint64_t> randomSorted( size_t n, uint64_t range, uint64_t base )
{
	std::vector<uint64_t> v;
	for( size_t i = 0; i < n * 2 && range; i++ ) v.push_back( base + rnd() % range );
	std::sort( v.begin(), v.end() );
	v.erase( std::unique( v.begin(), v.end() ), v.end() );
	if( v.size() > n ) v.resize( n );
	return v;
}
static void checkGroups( const std::vector<uint64_t>& mine, const std::vector<uint64_t>& other, size_t group, const char* what )
{
	for( size_t g0 = 0; g0 < mine.size(); g0 += group ) checkGroup( mine, g0, std::min( g0 + group, mine.size() ), other, what );
}
static void checkWindows()
{
	const std::vector<uint64_t> empty;
	for( int round = 0; round < 40; round++ )
	{
		const uint64_t range = 1ull << ( 6 + round % 12 );
		const std::vector<uint64_t> mine = randomSorted( 50 + rnd() % 900, range, 1000 ), other = randomSorted( 1 + rnd() % 900, range, 1000 );
		for( size_t group : { (size_t)1, (size_t)7, (size_t)64, (size_t)256 } )
		{
			checkGroups( mine, other, group, "random lists" );		 // about half of the codes shared where the range is small, windows at either end of `other`
			checkGroups( mine, mine, group, "identical lists" );	 // every code present: a window of exactly the group
			checkGroups( mine, empty, group, "an empty other list" ); // lo = hi = 0, nothing is read
		}
		// a group whose entries all lie below / above the other list: an empty window at its first / last end
		const std::vector<uint64_t> below = randomSorted( 300, 900, 0 ), above = randomSorted( 300, 900, 1000 + range + 5 );
		checkGroups( below, other, 256, "all below" );
		checkGroups( above, other, 256, "all above" );
		uint64_t lo, hi;
		combineWindow( other.data(), other.size(), below.front(), below.back(), &lo, &hi );
		CHECK( lo == 0 && hi == 0, "all below: window [%llu, %llu)", (unsigned long long)lo, (unsigned long long)hi );
		combineWindow( other.data(), other.size(), above.front(), above.back(), &lo, &hi );
		CHECK( lo == other.size() && hi == other.size(), "all above: window [%llu, %llu)", (unsigned long long)lo, (unsigned long long)hi );
		// a window of one: the group brackets exactly one entry of the other list
		const std::vector<uint64_t> one = { other[other.size() / 2] }, bracket = { one[0] - 1, one[0], one[0] + 1 };
		checkGroups( bracket, one, 256, "an other list of one" );
		checkGroups( one, other, 256, "a group of one" );
		combineWindow( other.data(), other.size(), one[0], one[0], &lo, &hi );
		CHECK( hi == lo && codeIndexInRange( other.data(), other.size(), lo, hi, one[0] ) == other.size() / 2, "a group of one present code: window [%llu, %llu)", (unsigned long long)lo,
			   (unsigned long long)hi );
	}
}

int main()
{
	checkTranslateSmall();
	checkTranslateBorders();
	checkWindows();
	if( g_failures )
	{
		printf( "%d combine host checks FAILED\n", g_failures );
		return 1;
	}
	printf( "combine host checks ok\n" );
	return 0;
}
