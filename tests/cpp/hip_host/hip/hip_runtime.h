// A stand-in <hip/hip_runtime.h> for building include/mvrt/device.hpp with a host compiler (tests/cpp/lane_walk_host.cpp): only what the header's
// text names.  No arithmetic lives here; the bit casts are memcpy.
#pragma once
#include <stdint.h>
#include <string.h>

#define __host__
#define __device__

struct float3
{
	float x, y, z;
};
struct uchar4
{
	unsigned char x, y, z, w;
};
struct uint2
{
	unsigned int x, y;
};
inline float3 make_float3( float x, float y, float z ) { return float3{ x, y, z }; }
inline uchar4 make_uchar4( unsigned int x, unsigned int y, unsigned int z, unsigned int w )
{
	return uchar4{ (unsigned char)x, (unsigned char)y, (unsigned char)z, (unsigned char)w };
}
inline uint2 make_uint2( unsigned int x, unsigned int y ) { return uint2{ x, y }; }
inline float __uint_as_float( unsigned int u )
{
	float f;
	memcpy( &f, &u, sizeof( f ) );
	return f;
}
inline unsigned int __float_as_uint( float f )
{
	unsigned int u;
	memcpy( &u, &f, sizeof( u ) );
	return u;
}
