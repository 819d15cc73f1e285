/*
 * Stand-in for MSVC's <intrin.h>, on the include path of the `ref` build only (oracle/Makefile).  The reference's vectorMath.hpp:20
 * includes <intrin.h> for the SSE4.1 floor/ceil intrinsics and voxCommon.hpp:116 calls _BitScanForward.  Our own text; DESIGN.md section 2
 * states what a stand-in may supply: declarations and bit-scan intrinsics, nothing that computes a value a test compares in floating point.
 */
#pragma once
#include <immintrin.h>

static inline unsigned char _BitScanForward( unsigned long* index, unsigned long mask )
{
	if( mask == 0 ) return 0;
	*index = (unsigned long)__builtin_ctzl( mask );
	return 1;
}
static inline unsigned char _BitScanReverse( unsigned long* index, unsigned long mask )
{
	if( mask == 0 ) return 0;
	*index = (unsigned long)( 8 * sizeof( unsigned long ) - 1 - __builtin_clzl( mask ) );
	return 1;
}
