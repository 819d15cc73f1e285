/*
 * Stand-in for <glm/glm.hpp>, on the include path of the `ref` build only (oracle/Makefile).  It exists so that the members of the reference's
 * IntersectorOctree class (IntersectorOctree.hpp:214-266) parse; oracle/ref_shim_walk.cpp never calls a member of that class, so no value
 * that a test compares passes through this arithmetic (the stand-in rule).  Our own text.
 */
#pragma once

namespace glm
{
struct vec3
{
	float x, y, z;
	vec3() : x( 0 ), y( 0 ), z( 0 ) {}
	explicit vec3( float s ) : x( s ), y( s ), z( s ) {}
	vec3( float a, float b, float c ) : x( a ), y( b ), z( c ) {}
};
inline vec3 operator+( const vec3& a, const vec3& b ) { return vec3( a.x + b.x, a.y + b.y, a.z + b.z ); }
inline vec3 operator*( const vec3& a, float s ) { return vec3( a.x * s, a.y * s, a.z * s ); }
} // namespace glm
