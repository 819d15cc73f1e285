// components_host.hip -- the helpers of csrc/voxel_passes.h that decide what the kernels of csrc/kernels_components.hip call adjacent (componentHalf,
// codeIndexIn on top of morphOffset / morphNeighbour), against brute force: the half of each element covers every unordered
// adjacent pair exactly once, the index-returning search on every subset order of small grids, and nothing is folded back at coordinates 0 and 2^21 - 1.  A
// program of its own: it makes no HIP call and needs no GPU.  Exit status 0 = every check held; each failure prints one line.
#include <stdio.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../massivevoxelraytracing_amd/csrc/voxel_passes.h"
#include "host_check.h"

// the half holds the offsets below (0, 0, 0) in the order (dz, dy, dx), and with every offset of the element exactly one of d and -d
static void checkHalves()
{
	for( int element = 0; element < 2; element++ )
	{
		const uint32_t nb = morphNeighbours( element );
		uint32_t inHalf = 0;
		for( uint32_t j = 0; j < nb; j++ )
		{
			int dx, dy, dz;
			morphOffset( element, j, dx, dy, dz );
			const bool below = dz < 0 || ( dz == 0 && ( dy < 0 || ( dy == 0 && dx < 0 ) ) );
			CHECK( componentHalf( element, j ) == below, "element %d j %u: offset (%d, %d, %d), half %d", element, j, dx, dy, dz, (int)componentHalf( element, j ) );
			inHalf += componentHalf( element, j ) ? 1u : 0u;
			uint32_t opposite = 0; // the neighbours of the element with the negated offset, and how many of the pair lie in the half
			for( uint32_t k = 0; k < nb; k++ )
			{
				int ex, ey, ez;
				morphOffset( element, k, ex, ey, ez );
				if( ex == -dx && ey == -dy && ez == -dz )
				{
					opposite++;
					CHECK( componentHalf( element, j ) != componentHalf( element, k ), "element %d: j %u and its opposite %u", element, j, k );
				}
			}
			CHECK( opposite == 1, "element %d j %u: %u opposites", element, j, opposite );
		}
		CHECK( inHalf * 2 == nb, "element %d: %u of %u in the half", element, inHalf, nb ); // 3 of 6, 13 of 26
	}
}

// a random subset of the grid of R = 2^levels: every unordered adjacent pair of voxels is reported exactly once by the walk the unite kernel makes, and
// codeIndexIn gives the position of every cell that is a voxel and n for every cell that is not
static void checkGrid( uint32_t levels, uint32_t percent )
{
	const uint32_t R = 1u << levels;
	std::vector<uint64_t> codes;
	for( uint32_t z = 0; z < R; z++ )
		for( uint32_t y = 0; y < R; y++ )
			for( uint32_t x = 0; x < R; x++ )
				if( rnd() % 100u < percent ) codes.push_back( encodeSlow( x, y, z ) );
	std::sort( codes.begin(), codes.end() );
	const uint64_t n = codes.size();
	for( uint32_t z = 0; z < R; z++ )
		for( uint32_t y = 0; y < R; y++ )
			for( uint32_t x = 0; x < R; x++ )
			{
				const uint64_t code = encodeSlow( x, y, z );
				uint64_t want = n;
				for( uint64_t i = 0; i < n; i++ )
					if( codes[i] == code ) want = i;
				const uint64_t got = codeIndexIn( codes.data(), n, code );
				CHECK( got == want, "levels %u %u%% cell (%u, %u, %u): index %llu, want %llu", levels, percent, x, y, z, (unsigned long long)got, (unsigned long long)want );
			}
	CHECK( codeIndexIn( codes.data(), 0, 0ull ) == 0, "empty list" );
	for( int element = 0; element < 2; element++ )
	{
		std::map<std::pair<uint64_t, uint64_t>, int> seen, want;
		for( uint64_t i = 0; i < n; i++ )
		{
			uint32_t x, y, z;
			mortonDecode( codes[i], x, y, z );
			for( uint32_t j = 0; j < morphNeighbours( element ); j++ )
			{
				uint64_t c;
				if( !componentHalf( element, j ) || !morphNeighbour( x, y, z, levels, element, j, &c ) ) continue;
				const uint64_t k = codeIndexIn( codes.data(), n, c );
				if( k < n ) seen[{ std::min( i, k ), std::max( i, k ) }]++;
			}
			for( uint64_t k = i + 1; k < n; k++ ) // brute force: every pair, by coordinate differences
			{
				uint32_t a, b, c;
				mortonDecode( codes[k], a, b, c );
				const int dx = abs( (int)a - (int)x ), dy = abs( (int)b - (int)y ), dz = abs( (int)c - (int)z );
				if( element == 0 ? dx + dy + dz == 1 : std::max( dx, std::max( dy, dz ) ) == 1 ) want[{ i, k }] = 1;
			}
		}
		CHECK( seen == want, "levels %u %u%% element %d: %zu pairs seen, %zu adjacent", levels, percent, element, seen.size(), want.size() );
	}
}

// voxels on the borders of the largest grid: the half-neighbours that exist are the ones signed arithmetic gives, found where they are voxels and nowhere else
static void checkNoFold()
{
	const uint32_t M = ( 1u << 21 ) - 1u, ys = 5u, zs = 9u;
	struct P
	{
		uint32_t x, y, z;
	};
	const P vox[] = { { 0, ys, zs }, { M, ys, zs }, { 0, ys + 1, zs }, { M, M, M }, { M - 1, M - 1, M }, { 0, 0, 0 }, { M, 0, 0 }, { 0, M, 0 }, { 0, 0, M } };
	std::vector<uint64_t> codes;
	for( const P& p : vox ) codes.push_back( encodeSlow( p.x, p.y, p.z ) );
	std::sort( codes.begin(), codes.end() );
	const uint64_t n = codes.size();
	for( int element = 0; element < 2; element++ )
	{
		uint32_t pairs = 0;
		for( const P& p : vox )
			for( uint32_t j = 0; j < morphNeighbours( element ); j++ )
			{
				int dx, dy, dz;
				morphOffset( element, j, dx, dy, dz );
				const int64_t nx = (int64_t)p.x + dx, ny = (int64_t)p.y + dy, nz = (int64_t)p.z + dz;
				const bool inside = nx >= 0 && nx <= M && ny >= 0 && ny <= M && nz >= 0 && nz <= M;
				uint64_t c = ~0ull;
				const bool got = morphNeighbour( p.x, p.y, p.z, 21, element, j, &c );
				CHECK( got == inside, "voxel (%u, %u, %u) element %d j %u: inside %d, got %d", p.x, p.y, p.z, element, j, (int)inside, (int)got );
				if( !got || !componentHalf( element, j ) ) continue;
				bool isVoxel = false;
				for( const P& q : vox ) isVoxel |= q.x == nx && q.y == ny && q.z == nz;
				const uint64_t k = codeIndexIn( codes.data(), n, c );
				CHECK( ( k < n ) == isVoxel, "voxel (%u, %u, %u) element %d j %u: found %d, voxel %d", p.x, p.y, p.z, element, j, (int)( k < n ), (int)isVoxel );
				pairs += k < n ? 1u : 0u;
			}
		// (0, ys, zs) + (0, ys + 1, zs) under both elements, the far corner pair under the cube alone; (0, ys, zs) and (M, ys, zs) never, nor (M, ys, zs) and (0, ys + 1, zs)
		CHECK( pairs == ( element ? 2u : 1u ), "element %d: %u pairs on the borders", element, pairs );
	}
}

int main()
{
	checkHalves();
	for( uint32_t levels : { 1u, 2u } ) // gridRes 2 and 4
		for( uint32_t percent : { 20u, 50u, 80u, 100u } )
			for( int k = 0; k < 8; k++ ) checkGrid( levels, percent );
	checkNoFold();
	if( g_failures ) printf( "%d check(s) failed\n", g_failures );
	else printf( "components host checks ok\n" );
	return g_failures ? 1 : 0;
}
