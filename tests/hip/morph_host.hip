// morph_host.hip -- the structuring-element helpers of csrc/voxel_passes.h (morphNeighbours, morphOffset, morphNeighbour, codePresentIn, morphEmptyMask), the
// host-callable twins of what the kernels of csrc/kernels_morph.hip ask per voxel, against brute force: the offset tables, the in-grid test at
// every border up to gridRes 2^21, and the masks of random sets against a dense grid.  A program of its own: it makes no HIP call and needs no GPU.  Exit status
// 0 = every check held; each failure prints one line.
#include <stdio.h>

#include <algorithm>
#include <set>
#include <vector>

#include "../../massivevoxelraytracing_amd/csrc/voxel_passes.h"
#include "host_check.h"

static void checkOffsets()
{
	for( int element = 0; element < 2; element++ )
	{
		const uint32_t nb = morphNeighbours( element );
		CHECK( nb == ( element ? 26u : 6u ), "element %d has %u neighbours", element, nb );
		std::set<int> seen;
		for( uint32_t j = 0; j < nb; j++ )
		{
			int dx = 9, dy = 9, dz = 9;
			morphOffset( element, j, dx, dy, dz );
			CHECK( dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && dz >= -1 && dz <= 1, "element %d j %u: offset (%d, %d, %d)", element, j, dx, dy, dz );
			const int manhattan = abs( dx ) + abs( dy ) + abs( dz );
			CHECK( element ? manhattan >= 1 : manhattan == 1, "element %d j %u: offset (%d, %d, %d)", element, j, dx, dy, dz );
			seen.insert( ( dz + 1 ) * 9 + ( dy + 1 ) * 3 + dx + 1 );
		}
		CHECK( seen.size() == nb, "element %d: %zu distinct offsets of %u", element, seen.size(), nb ); // all different: the whole element
	}
	CHECK( morphElementOk( 0 ) && morphElementOk( 1 ) && !morphElementOk( 2 ) && !morphElementOk( -1 ), "morphElementOk" );
}

// every neighbour of a cell against signed 64-bit arithmetic
static void checkCell( uint32_t levels, uint32_t x, uint32_t y, uint32_t z )
{
	const int64_t R = (int64_t)1 << levels;
	for( int element = 0; element < 2; element++ )
		for( uint32_t j = 0; j < morphNeighbours( element ); j++ )
		{
			int dx, dy, dz;
			morphOffset( element, j, dx, dy, dz );
			const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy, nz = (int64_t)z + dz;
			const bool inside = nx >= 0 && nx < R && ny >= 0 && ny < R && nz >= 0 && nz < R;
			uint64_t code = ~0ull;
			const bool got = morphNeighbour( x, y, z, levels, element, j, &code );
			CHECK( got == inside, "levels %u cell (%u, %u, %u) element %d j %u: inside %d, got %d", levels, x, y, z, element, j, (int)inside, (int)got );
			if( got && inside )
				CHECK( code == encodeSlow( (uint32_t)nx, (uint32_t)ny, (uint32_t)nz ), "levels %u cell (%u, %u, %u) element %d j %u: code %llx", levels, x, y, z, element, j,
					   (unsigned long long)code );
		}
}
static void checkBorders()
{
	for( uint32_t levels : { 1u, 2u, 3u, 8u, 20u, 21u } )
	{
		const uint32_t R = 1u << levels;
		const uint32_t edge[4] = { 0u, 1u % R, R - 2u < R ? R - 2u : 0u, R - 1u };
		for( uint32_t a : edge )
			for( uint32_t b : edge )
				for( uint32_t c : edge ) checkCell( levels, a, b, c ); // every corner, edge and face of the grid and the cells next to them
		for( int k = 0; k < 200; k++ ) checkCell( levels, (uint32_t)( rnd() % R ), (uint32_t)( rnd() % R ), (uint32_t)( rnd() % R ) );
	}
}

// the masks of a random set against a dense grid
static void checkMasks( uint32_t levels, uint32_t percent )
{
	const uint32_t R = 1u << levels;
	std::vector<uint8_t> grid( (size_t)R * R * R, 0 );
	std::vector<uint64_t> codes;
	for( uint32_t z = 0; z < R; z++ )
		for( uint32_t y = 0; y < R; y++ )
			for( uint32_t x = 0; x < R; x++ )
				if( rnd() % 100u < percent )
				{
					grid[( (size_t)z * R + y ) * R + x] = 1;
					codes.push_back( encodeSlow( x, y, z ) );
				}
	std::sort( codes.begin(), codes.end() );
	auto at = [&]( int64_t x, int64_t y, int64_t z ) { return grid[( (size_t)z * R + (size_t)y ) * R + (size_t)x] != 0; };
	for( uint32_t z = 0; z < R; z++ )
		for( uint32_t y = 0; y < R; y++ )
			for( uint32_t x = 0; x < R; x++ )
			{
				const uint64_t code = encodeSlow( x, y, z );
				CHECK( codePresentIn( codes.data(), codes.size(), code ) == at( x, y, z ), "levels %u cell (%u, %u, %u): codePresentIn", levels, x, y, z );
				if( !at( x, y, z ) ) continue;
				for( int element = 0; element < 2; element++ )
				{
					uint32_t want = 0;
					for( uint32_t j = 0; j < morphNeighbours( element ); j++ )
					{
						int dx, dy, dz;
						morphOffset( element, j, dx, dy, dz );
						const int64_t nx = (int64_t)x + dx, ny = (int64_t)y + dy, nz = (int64_t)z + dz;
						if( nx < 0 || ny < 0 || nz < 0 || nx >= R || ny >= R || nz >= R ) continue; // outside the grid: occupied
						if( !at( nx, ny, nz ) ) want |= 1u << j;
					}
					const uint32_t got = morphEmptyMask( codes.data(), codes.size(), levels, element, code );
					CHECK( got == want, "levels %u %u%% cell (%u, %u, %u) element %d: mask %08x, want %08x", levels, percent, x, y, z, element, got, want );
				}
			}
	// an empty list: every in-grid neighbour is empty
	const uint32_t all = morphEmptyMask( codes.data(), 0, levels, 1, encodeSlow( R / 2, R / 2, R / 2 ) );
	CHECK( all == ( levels == 1 ? all : 0x3FFFFFFu ), "empty list: mask %08x", all );
}

int main()
{
	checkOffsets();
	checkBorders();
	for( uint32_t levels : { 1u, 2u, 3u, 4u } )
		for( uint32_t percent : { 10u, 50u, 90u, 100u } ) checkMasks( levels, percent );
	// a single voxel in each corner of the largest grid: the neighbours that exist, and no wrap in the 21 bits per axis
	for( uint32_t corner = 0; corner < 8; corner++ )
	{
		const uint32_t M = ( 1u << 21 ) - 1u, x = corner & 1u ? M : 0u, y = corner & 2u ? M : 0u, z = corner & 4u ? M : 0u;
		const uint64_t code = encodeSlow( x, y, z );
		CHECK( __builtin_popcount( morphEmptyMask( &code, 1, 21, 0, code ) ) == 3, "corner %u: faces", corner );
		CHECK( __builtin_popcount( morphEmptyMask( &code, 1, 21, 1, code ) ) == 7, "corner %u: cube", corner );
	}
	if( g_failures ) printf( "%d check(s) failed\n", g_failures );
	else printf( "morph host checks ok\n" );
	return g_failures ? 1 : 0;
}
