/*
 * Stand-in for <glm/glm.hpp>, on the include path of the `ref` build only (oracle/Makefile).  It exists so that the members of the reference's
 * IntersectorOctree class (IntersectorOctree.hpp:214-266) and CameraPinhole::initFromPerspective (renderCommon.hpp:21-35) parse;
 * oracle/ref_shim_walk.cpp never calls a member of that class and oracle/ref_shim_render.cpp never calls initFromPerspective, so no value that a
 * test compares passes through this arithmetic (the stand-in rule).  Our own text.
 */
#pragma once

namespace glm
{
struct vec4
{
	float x, y, z, w;
	vec4() : x( 0 ), y( 0 ), z( 0 ), w( 0 ) {}
	vec4( float a, float b, float c, float d ) : x( a ), y( b ), z( c ), w( d ) {}
	float& operator[]( int i ) { return ( &x )[i]; }
	const float& operator[]( int i ) const { return ( &x )[i]; }
};
struct vec3
{
	float x, y, z;
	vec3() : x( 0 ), y( 0 ), z( 0 ) {}
	explicit vec3( float s ) : x( s ), y( s ), z( s ) {}
	vec3( float a, float b, float c ) : x( a ), y( b ), z( c ) {}
	explicit vec3( const vec4& v ) : x( v.x ), y( v.y ), z( v.z ) {}
	float& operator[]( int i ) { return ( &x )[i]; }
	const float& operator[]( int i ) const { return ( &x )[i]; }
};
inline vec3 operator+( const vec3& a, const vec3& b ) { return vec3( a.x + b.x, a.y + b.y, a.z + b.z ); }
inline vec3 operator*( const vec3& a, float s ) { return vec3( a.x * s, a.y * s, a.z * s ); }

// column-major, as glm: m[c] is column c
struct mat4
{
	vec4 col[4];
	vec4& operator[]( int c ) { return col[c]; }
	const vec4& operator[]( int c ) const { return col[c]; }
};
struct mat3
{
	vec3 col[3];
	mat3() {}
	explicit mat3( const mat4& m )
	{
		for( int c = 0; c < 3; c++ ) col[c] = vec3( m[c] );
	}
	vec3& operator[]( int c ) { return col[c]; }
	const vec3& operator[]( int c ) const { return col[c]; }
};
inline mat3 transpose( const mat3& m )
{
	mat3 t;
	for( int c = 0; c < 3; c++ )
		for( int r = 0; r < 3; r++ ) t[c][r] = m[r][c];
	return t;
}
inline vec3 operator*( const mat3& m, const vec3& v ) { return m[0] * v.x + m[1] * v.y + m[2] * v.z; }
} // namespace glm
