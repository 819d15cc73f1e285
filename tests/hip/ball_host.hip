// ball_host.hip -- the round-offset helpers of csrc/voxel_passes.h (ballReach, ballShiftRange, ballShifted, ballKey, ballShiftKey), the host-callable twins of what
// the kernels of csrc/kernels_ball.hip ask per entry and per record, against brute force: the reach of every legal radius, the shift interval and
// the shifted code at every border up to gridRes 2^21, and the three passes themselves, run here on std::map with exactly these helpers, against the minimum over
// all voxels of ( distance, index ) on random sets.  A program of its own: it makes no HIP call and needs no GPU.  Exit status 0 = every check held; each failure
// prints one line.
#include <stdio.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../massivevoxelraytracing_amd/csrc/voxel_passes.h"
#include "host_check.h"

static void checkReachAndKeys()
{
	for( uint32_t rho = 0; rho <= 1100u; rho++ )
	{
		uint32_t k = 0;
		while( ( k + 1u ) * ( k + 1u ) <= rho ) k++;
		CHECK( ballReach( rho ) == k, "rho %u: reach %u, want %u", rho, ballReach( rho ), k );
	}
	CHECK( ballReach( 1024u ) == 32u, "the largest reach" );
	for( int t = 0; t < 1000; t++ )
	{
		const uint32_t d2 = (uint32_t)( rnd() % 1025u ), p = (uint32_t)rnd(), d3 = (uint32_t)( rnd() % 1025u ), q = (uint32_t)rnd();
		const uint64_t a = ballKey( d2, p ), b = ballKey( d3, q );
		CHECK( ballKeyDist2( a ) == d2 && ballKeyPayload( a ) == p, "key fields" );
		CHECK( ( a < b ) == ( d2 < d3 || ( d2 == d3 && p < q ) ), "keys order by ( d2, payload )" );
		const int32_t s = (int32_t)( rnd() % 65u ) - 32;
		CHECK( ballKeyDist2( ballShiftKey( a, s ) ) == d2 + (uint32_t)( s * s ) && ballKeyPayload( ballShiftKey( a, s ) ) == p, "shifted key" );
		CHECK( ( ballShiftKey( a, s ) < ballShiftKey( b, s ) ) == ( a < b ), "a shift keeps the order" );
	}
}

// the interval and every shifted code of a cell against signed 64-bit arithmetic
static void checkCell( uint32_t levels, uint32_t x, uint32_t y, uint32_t z, uint32_t d2, uint32_t rho )
{
	const int64_t R = (int64_t)1 << levels;
	const uint32_t xyz[3] = { x, y, z };
	const uint64_t code = encodeSlow( x, y, z );
	for( uint32_t axis = 0; axis < 3; axis++ )
	{
		CHECK( ballAxisCoord( code, axis ) == xyz[axis], "levels %u cell (%u, %u, %u) axis %u: coordinate %u", levels, x, y, z, axis, ballAxisCoord( code, axis ) );
		int32_t first = 99;
		const uint32_t count = ballShiftRange( xyz[axis], levels, d2, rho, &first );
		uint32_t want = 0;
		int32_t wantFirst = 0;
		bool any = false;
		for( int32_t s = -33; s <= 33; s++ )
		{
			int64_t c[3] = { x, y, z };
			c[axis] += s;
			const bool inside = c[axis] >= 0 && c[axis] < R;
			uint64_t got = ~0ull;
			const bool ok = ballShifted( code, levels, axis, s, &got );
			CHECK( ok == inside, "levels %u cell (%u, %u, %u) axis %u shift %d: inside %d, got %d", levels, x, y, z, axis, s, (int)inside, (int)ok );
			if( ok && inside ) CHECK( got == encodeSlow( (uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2] ), "levels %u cell (%u, %u, %u) axis %u shift %d: code", levels, x, y, z, axis, s );
			if( inside && (int64_t)d2 + (int64_t)s * s <= (int64_t)rho )
			{
				if( !any ) wantFirst = s;
				any = true;
				want++;
			}
		}
		CHECK( count == want && first == wantFirst, "levels %u cell (%u, %u, %u) axis %u d2 %u rho %u: [%d, +%u), want [%d, +%u)", levels, x, y, z, axis, d2, rho, first, count,
			   wantFirst, want );
	}
}
static void checkBorders()
{
	for( uint32_t levels : { 1u, 2u, 3u, 5u, 8u, 20u, 21u } )
	{
		const uint32_t R = 1u << levels;
		const uint32_t edge[6] = { 0u, 1u % R, 31u % R, R - 32u < R ? R - 32u : 0u, R - 2u < R ? R - 2u : 0u, R - 1u };
		for( uint32_t rho : { 1u, 2u, 3u, 4u, 9u, 1023u, 1024u } )
		{
			for( uint32_t a : edge )
				for( uint32_t b : edge ) checkCell( levels, a, b, edge[( a + b ) % 6u], 0u, rho );
			for( int t = 0; t < 50; t++ ) checkCell( levels, (uint32_t)( rnd() % R ), (uint32_t)( rnd() % R ), (uint32_t)( rnd() % R ), (uint32_t)( rnd() % ( rho + 1u ) ), rho );
		}
	}
}

// the three passes on a map, with the helpers the kernels use: entries ( code -> smallest key ), every entry sends a record to each shift of its interval
typedef std::map<uint64_t, uint64_t> Cells;
static Cells bandOf( const Cells& seeds, uint32_t levels, uint32_t rho )
{
	Cells cur = seeds;
	for( uint32_t axis = 0; axis < 3; axis++ )
	{
		Cells next;
		for( const auto& e : cur )
		{
			int32_t first = 0;
			const uint32_t count = ballShiftRange( ballAxisCoord( e.first, axis ), levels, ballKeyDist2( e.second ), rho, &first );
			for( uint32_t j = 0; j < count; j++ )
			{
				uint64_t c = 0;
				CHECK( ballShifted( e.first, levels, axis, first + (int32_t)j, &c ), "a shift of the interval leaves the grid" );
				const uint64_t k = ballShiftKey( e.second, first + (int32_t)j );
				CHECK( ballKeyDist2( k ) <= rho, "a record beyond rho" );
				auto it = next.find( c );
				if( it == next.end() ) next[c] = k;
				else if( k < it->second ) it->second = k;
			}
		}
		cur.swap( next );
	}
	return cur;
}
static void checkBand( uint32_t levels, uint32_t percent, uint32_t rho )
{
	const uint32_t R = 1u << levels;
	std::vector<uint64_t> codes;
	for( uint32_t z = 0; z < R; z++ )
		for( uint32_t y = 0; y < R; y++ )
			for( uint32_t x = 0; x < R; x++ )
				if( rnd() % 100u < percent ) codes.push_back( encodeSlow( x, y, z ) );
	if( codes.empty() ) codes.push_back( encodeSlow( R / 2, R / 2, R / 2 ) );
	std::sort( codes.begin(), codes.end() );
	// the seeds of the dilation: the voxels with an empty in-grid face neighbour, payload = the index.  The seeds of the erosion: the cells of one FACES step
	Cells outer, inner;
	for( size_t i = 0; i < codes.size(); i++ )
	{
		const uint32_t mask = morphEmptyMask( codes.data(), codes.size(), levels, 0, codes[i] );
		if( mask ) outer[codes[i]] = ballKey( 0u, (uint32_t)i );
		uint32_t x, y, z;
		mortonDecode( codes[i], x, y, z );
		for( uint32_t j = 0; j < 6; j++ )
		{
			uint64_t c;
			if( ( mask >> j & 1u ) && morphNeighbour( x, y, z, levels, 0, j, &c ) ) inner[c] = ballKey( 0u, 0u );
		}
	}
	const Cells grown = bandOf( outer, levels, rho ), shrunk = bandOf( inner, levels, rho );
	for( uint32_t z = 0; z < R; z++ )
		for( uint32_t y = 0; y < R; y++ )
			for( uint32_t x = 0; x < R; x++ )
			{
				const uint64_t c = encodeSlow( x, y, z );
				const bool voxel = codePresentIn( codes.data(), codes.size(), c );
				uint64_t best = ~0ull; // over the voxels ( distance, index ), or over the empty cells ( distance, 0 )
				for( uint32_t w = 0; w < R; w++ )
					for( uint32_t v = 0; v < R; v++ )
						for( uint32_t u = 0; u < R; u++ )
						{
							const uint64_t o = encodeSlow( u, v, w );
							const uint64_t i = codeIndexIn( codes.data(), codes.size(), o );
							if( ( i < codes.size() ) == voxel ) continue;
							const int64_t dx = (int64_t)u - x, dy = (int64_t)v - y, dz = (int64_t)w - z;
							const uint64_t k = ballKey( (uint32_t)( dx * dx + dy * dy + dz * dz ), voxel ? 0u : (uint32_t)i );
							best = k < best ? k : best;
						}
				const Cells& band = voxel ? shrunk : grown;
				const auto it = band.find( c );
				const bool within = best != ~0ull && ballKeyDist2( best ) <= rho;
				CHECK( ( it != band.end() ) == within, "levels %u %u%% rho %u cell (%u, %u, %u) voxel %d: in the band %d, want %d", levels, percent, rho, x, y, z, (int)voxel,
					   (int)( it != band.end() ), (int)within );
				if( it != band.end() && within )
					CHECK( it->second == best, "levels %u %u%% rho %u cell (%u, %u, %u) voxel %d: key %llx, want %llx", levels, percent, rho, x, y, z, (int)voxel,
						   (unsigned long long)it->second, (unsigned long long)best );
			}
}

int main()
{
	checkReachAndKeys();
	checkBorders();
	for( uint32_t percent : { 2u, 30u, 90u } )
		for( uint32_t rho : { 1u, 2u, 3u, 4u, 5u, 9u, 14u } ) checkBand( 3, percent, rho );
	checkBand( 4, 3u, 14u ); // sparse in a larger grid: the full reach of the ball is inside
	checkBand( 2, 100u, 5u ); // a full grid: no seed, no band
	if( g_failures ) printf( "%d check(s) failed\n", g_failures );
	else printf( "ball host checks ok\n" );
	return g_failures ? 1 : 0;
}
