// host_check.h -- what the host programs tests/hip/*_host.hip share: CHECK and its failure count (the first 20 failures print one line each; main returns
// non-zero when g_failures is), the xorshift64 generator behind their random cases, and the Morton code of a cell bit by bit.  A program whose cases were
// generated from another seed defines HOST_CHECK_SEED before it includes this.
#pragma once
#include <stdint.h>
#include <stdio.h>

static int g_failures = 0;
#define CHECK( cond, ... )                     \
	do                                         \
	{                                          \
		if( !( cond ) )                        \
		{                                      \
			if( g_failures++ < 20 )            \
			{                                  \
				printf( "FAILED %s: ", #cond ); \
				printf( __VA_ARGS__ );         \
				printf( "\n" );                \
			}                                  \
		}                                      \
	} while( 0 )

#ifndef HOST_CHECK_SEED
#define HOST_CHECK_SEED 0x9E3779B97F4A7C15ull
#endif
static uint64_t g_rng = HOST_CHECK_SEED;
static uint64_t rnd() // xorshift64
{
	g_rng ^= g_rng << 13;
	g_rng ^= g_rng >> 7;
	g_rng ^= g_rng << 17;
	return g_rng;
}

// brute force: the code of (x, y, z) bit by bit
static uint64_t encodeSlow( uint64_t x, uint64_t y, uint64_t z )
{
	uint64_t c = 0;
	for( int b = 0; b < 21; b++ ) c |= ( ( x >> b ) & 1ull ) << ( 3 * b ) | ( ( y >> b ) & 1ull ) << ( 3 * b + 1 ) | ( ( z >> b ) & 1ull ) << ( 3 * b + 2 );
	return c;
}
