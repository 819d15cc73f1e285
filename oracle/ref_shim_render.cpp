/*
 * ref_shim_render.cpp -- C entry points over the HOST branch of the REFERENCE's renderer headers, compiled as they lie with ROCm's host clang++
 * in MS-compatibility mode: renderCommon.hpp (CameraPinhole::shoot / shootThinLens, PCG32, uniformf, GetOrthonormalBasis, sampleLambertian,
 * degammaReflectance / rawReflectance, luminance, getSpherical, upper_bound_f, HDRI::importanceSample and its table readers, LCGShuffler) and
 * pmjSampler.hpp (GetPMJ02Samples through PMJSampler::setup( false, ... ), sample2d, nested_uniform_scramble, scramble_f32).  voxCommon.hpp comes
 * first: pmjSampler.hpp calls its hashCombine without including it.  This file contains no reference code; it includes the headers from $(REF) at
 * build time (oracle/Makefile, target `ref`) and the library lives only in oracle/_ref/ (git-ignored).
 *
 * The stand-in rule: oracle/standin/ supplies <intrin.h>, <glm/glm.hpp> and "Orochi/Orochi.h".  No value that a test
 * compares passes through stand-in code, so nothing here calls CameraPinhole::initFromPerspective (the stand-in glm would do its arithmetic: the
 * 15 camera floats come from the caller), HDRI::load / loadPrimary / cleanUp (Orochi; the reference builds its tables in voxKernel.cu, which no
 * host compiler builds: the seven tables come from the caller), PMJSampler::setup( true, ... ), or the constructor of Buffer or Shader.
 *
 * Transcendentals (sinf, cosf, atan2f, powf) are those of the C library this is linked against, not of the reference's own build (MSVC's CRT).
 * The device-only HDRI::sampleNearest is not in the host branch and is not here.
 * TEST INFRASTRUCTURE: used by tests/test_reference_pins_cpu.py and tests/test_gpu_reference_pins.py.
 */
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "voxCommon.hpp"
#include "renderCommon.hpp"
#include "pmjSampler.hpp"

#define SHIM_API extern "C" __attribute__( ( visibility( "default" ) ) )

static inline float3 f3( const float* p ) { return float3{ p[0], p[1], p[2] }; }
static inline void put3( float* p, float3 v )
{
	p[0] = v.x;
	p[1] = v.y;
	p[2] = v.z;
}

SHIM_API int refr_struct_sizes( int* out )
{
	out[0] = (int)sizeof( CameraPinhole );
	out[1] = (int)sizeof( PCG32 );
	out[2] = (int)PMJSampler::LENGTH;
	out[3] = (int)PMJSampler::N_SEQUENCE;
	return 4;
}

// cam15: m_o, m_front, m_up, m_right, m_tanHthetaY, m_lensR, m_focus in declaration order.  px: n * 4 ints (x, y, imageWidth, imageHeight);
// fl: n * 4 floats (xoffsetInPixel, yoffsetInPixel, u0, u1).  thinLens == 0: shoot (u0, u1 unused); else shootThinLens.
SHIM_API void refr_camera_shoot( const float* cam15, int64_t n, const int32_t* px, const float* fl, int thinLens, float* ro, float* rd )
{
	CameraPinhole c;
	c.m_o = f3( cam15 );
	c.m_front = f3( cam15 + 3 );
	c.m_up = f3( cam15 + 6 );
	c.m_right = f3( cam15 + 9 );
	c.m_tanHthetaY = cam15[12];
	c.m_lensR = cam15[13];
	c.m_focus = cam15[14];
	for( int64_t i = 0; i < n; i++ )
	{
		const int32_t* p = px + i * 4;
		const float* f = fl + i * 4;
		float3 o, d;
		if( thinLens )
			c.shootThinLens( &o, &d, p[0], p[1], f[0], f[1], p[2], p[3], f[2], f[3] );
		else
			c.shoot( &o, &d, p[0], p[1], f[0], f[1], p[2], p[3] );
		put3( ro + i * 3, o );
		put3( rd + i * 3, d );
	}
}

SHIM_API void refr_pcg32( uint64_t seed, uint64_t stream, int64_t n, uint32_t* out )
{
	PCG32 rng;
	rng.setup( seed, stream );
	for( int64_t i = 0; i < n; i++ ) out[i] = rng.nextU32();
}
SHIM_API void refr_uniformf( int64_t n, const uint32_t* x, float* out )
{
	for( int64_t i = 0; i < n; i++ ) out[i] = uniformf( x[i] );
}
SHIM_API void refr_orthonormal_basis( int64_t n, const float* z, float* xaxis, float* yaxis )
{
	for( int64_t i = 0; i < n; i++ )
	{
		float3 x, y;
		GetOrthonormalBasis( f3( z + i * 3 ), &x, &y );
		put3( xaxis + i * 3, x );
		put3( yaxis + i * 3, y );
	}
}
// ab: n * 2 floats
SHIM_API void refr_sample_lambertian( int64_t n, const float* ab, const float* Ng, float* out )
{
	for( int64_t i = 0; i < n; i++ ) put3( out + i * 3, sampleLambertian( ab[i * 2], ab[i * 2 + 1], f3( Ng + i * 3 ) ) );
}
SHIM_API void refr_get_spherical( int64_t n, const float* dir, float* out2 )
{
	for( int64_t i = 0; i < n; i++ )
	{
		float2 s = getSpherical( f3( dir + i * 3 ) );
		out2[i * 2] = s.x;
		out2[i * 2 + 1] = s.y;
	}
}
// rgba: n * 4 bytes
SHIM_API void refr_reflectance( int64_t n, const uint8_t* rgba, float* degamma, float* raw )
{
	for( int64_t i = 0; i < n; i++ )
	{
		uchar4 c = { rgba[i * 4], rgba[i * 4 + 1], rgba[i * 4 + 2], rgba[i * 4 + 3] };
		put3( degamma + i * 3, degammaReflectance( c ) );
		put3( raw + i * 3, rawReflectance( c ) );
	}
}
SHIM_API void refr_luminance( int64_t n, const float* rgb, float* out )
{
	for( int64_t i = 0; i < n; i++ ) out[i] = luminance( f3( rgb + i * 3 ) );
}
// upper_bound_f over f( i ) = values[i], once per b
SHIM_API void refr_upper_bound( const float* values, int nValues, int64_t n, const float* b, int32_t* out )
{
	for( int64_t i = 0; i < n; i++ ) out[i] = upper_bound_f( [values]( int k ) { return values[k]; }, nValues, b[i] );
}
// LCGShuffler::tryInit( r0, r1, numberOfElement ), then operator() on every index; returns tryInit's answer
SHIM_API int refr_lcg_shuffler( uint32_t r0, uint32_t r1, uint32_t numberOfElement, int64_t n, const uint32_t* idx, uint32_t* out )
{
	LCGShuffler s;
	bool ok = s.tryInit( r0, r1, numberOfElement );
	for( int64_t i = 0; i < n; i++ ) out[i] = s( idx[i] );
	return ok ? 1 : 0;
}

// PMJSampler::setup( false, 0 ): the host table, 2 * LENGTH * N_SEQUENCE floats
SHIM_API void refr_pmj_table( float* out )
{
	PMJSampler s;
	s.setup( false, 0 );
	std::copy( s.m_samples, s.m_samples + 2 * PMJSampler::LENGTH * PMJSampler::N_SEQUENCE, out );
	free( s.m_samples );
	s.m_samples = 0;
}
// sample2d on the caller's table
SHIM_API void refr_pmj_sample2d( const float* table, int64_t n, const uint32_t* sampleIdx, const uint32_t* dimension, const uint32_t* stream, float* out2 )
{
	PMJSampler s;
	s.m_samples = const_cast<float*>( table );
	for( int64_t i = 0; i < n; i++ )
	{
		float2 v = s.sample2d( sampleIdx[i], dimension[i], stream[i] );
		out2[i * 2] = v.x;
		out2[i * 2 + 1] = v.y;
	}
	s.m_samples = 0;
}
SHIM_API void refr_nested_uniform_scramble( int64_t n, const uint32_t* x, const uint32_t* seed, uint32_t* out )
{
	for( int64_t i = 0; i < n; i++ ) out[i] = nested_uniform_scramble( x[i], seed[i] );
}
SHIM_API void refr_scramble_f32( int64_t n, const float* x, const uint32_t* seed, float* out )
{
	for( int64_t i = 0; i < n; i++ ) out[i] = scramble_f32( x[i], seed[i] );
}

// An HDRI over the caller's pixels (w * h float4) and seven tables (tables7: uniform, +x, -x, +y, -y, +z, -z; w * h uint32 each).
struct ShimHDRI
{
	HDRI hdri;
	std::vector<float4> pixels; // float4 is alignas( 16 ): a copy, whatever the caller's alignment
	ShimHDRI( const float* rgba, int w, int h, const uint32_t* const* tables7, float scale ) : pixels( (size_t)w * h )
	{
		for( size_t i = 0; i < pixels.size(); i++ ) pixels[i] = float4{ rgba[i * 4], rgba[i * 4 + 1], rgba[i * 4 + 2], rgba[i * 4 + 3] };
		hdri.m_pixels = pixels.data();
		hdri.m_sat = const_cast<uint32_t*>( tables7[0] );
		for( int i = 0; i < 6; i++ ) hdri.m_sats[i] = const_cast<uint32_t*>( tables7[i + 1] );
		hdri.m_width = w;
		hdri.m_height = h;
		hdri.m_scale = scale;
	}
};
// N: n * 3, u: n * 4 (u0 .. u3).  The caller answers for the tables: one without a total makes the reference index out of range.
SHIM_API void refr_hdri_importance_sample( const float* rgba, int w, int h, const uint32_t* const* tables7, float scale, int64_t n, const float* N, int axisAligned,
										   const float* u, float* direction, float* L, float* srPDF )
{
	ShimHDRI s( rgba, w, h, tables7, scale );
	for( int64_t i = 0; i < n; i++ )
	{
		float3 d, l;
		s.hdri.importanceSample( &d, &l, srPDF + i, f3( N + i * 3 ), axisAligned != 0, u[i * 4], u[i * 4 + 1], u[i * 4 + 2], u[i * 4 + 3] );
		put3( direction + i * 3, d );
		put3( L + i * 3, l );
	}
}
// getPrefixSumExclusiveH( table, x ), getPrefixSumExclusiveV( table, x, y ) and getCount( table, x, y ) at n points xy (n * 2 uint32);
// x <= w (H only reads x - 1), and x < w, y < h for getCount / y <= h for V are the caller's to keep: out-of-range points give 0 here.
SHIM_API void refr_hdri_table_queries( const uint32_t* table, int w, int h, int64_t n, const uint32_t* xy, uint32_t* prefixH, uint32_t* prefixV, uint32_t* count )
{
	HDRI hdri;
	hdri.m_width = w;
	hdri.m_height = h;
	for( int64_t i = 0; i < n; i++ )
	{
		uint32_t x = xy[i * 2], y = xy[i * 2 + 1];
		prefixH[i] = x <= (uint32_t)w ? hdri.getPrefixSumExclusiveH( table, x ) : 0;
		prefixV[i] = ( x < (uint32_t)w && y <= (uint32_t)h ) ? hdri.getPrefixSumExclusiveV( table, x, y ) : 0;
		count[i] = ( x < (uint32_t)w && y < (uint32_t)h ) ? hdri.getCount( table, x, y ) : 0;
	}
}
