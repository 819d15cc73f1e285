/*
 * ref_shim_walk.cpp -- C entry points over the four REFERENCE headers that compile as they lie with ROCm's host clang++ in MS-compatibility
 * mode: voxCommon.hpp (traversal, embedMask, getHitN, bSearch, hashCombine, numberOfSortBitsMorton), voxelization.hpp (VTContext), morton.hpp
 * and IntersectorOctree.hpp (buildOctreeDAGReference, buildOctreeNaive).  This file contains no reference code; it includes the headers from
 * $(REF) at build time (oracle/Makefile, target `ref`) and the library lives only in oracle/_ref/ (git-ignored).
 *
 * The stand-in rule: oracle/standin/ supplies <intrin.h> and <glm/glm.hpp>, declarations and bit scans only.  No value
 * that a test compares passes through stand-in arithmetic, so everything here calls the reference's free functions with bounds the caller
 * passes in and never goes through IntersectorOctree::build, whose m_upper our glm::vec3 would compute.
 *
 * MS-compatibility mode cannot compile glibc's <string.h> at -O2, so nothing here includes it: std::copy, not memcpy.
 * TEST INFRASTRUCTURE: used by tests/test_reference_pins_cpu.py and tests/test_gpu_reference_pins.py.
 */
#include <stdint.h>
#include <algorithm>
#include <cassert>
#include <map>
#include <vector>

#include "morton.hpp"
#include "voxCommon.hpp"
#include "voxelization.hpp"
#include "IntersectorOctree.hpp"

#define SHIM_API extern "C" __attribute__( ( visibility( "default" ) ) )

SHIM_API int refw_struct_sizes( int* out )
{
	out[0] = (int)sizeof( OctreeNode );
	out[1] = (int)sizeof( StackElement );
	out[2] = (int)sizeof( OctreeTask );
	out[3] = (int)sizeof( VoxelAttirb );
	return 4;
}

// The triangle loop of the reference exists only in its .cpp / .cu files; restated here from voxKernel.cu:109-146 (== voxRT.cpp:198-240) the
// way oracle/mvrt_oracle.cpp restates it: x range, y range per x, z range per (x, y), the plane test, then the magic-bits Morton code.
// tris: nTri * 9 floats.  countsOut: voxels per triangle.  Returns the total; fills mortonOut up to `capacity` (null / 0 to count only).
SHIM_API int64_t refw_voxelize( const float* tris, int64_t nTri, int sixSeparating, const float* origin3, float dps, int gridRes, uint32_t* countsOut,
								uint64_t* mortonOut, int64_t capacity )
{
	const bool six = sixSeparating != 0;
	const float3 origin = { origin3[0], origin3[1], origin3[2] };
	int64_t n = 0;
	for( int64_t t = 0; t < nTri; t++ )
	{
		const float* v = tris + t * 9;
		VTContext context( float3{ v[0], v[1], v[2] }, float3{ v[3], v[4], v[5] }, float3{ v[6], v[7], v[8] }, six, origin, dps, gridRes );
		const int64_t before = n;
		int2 xrange = context.xRangeInclusive();
		for( int x = xrange.x; x <= xrange.y; x++ )
		{
			int2 yrange = context.yRangeInclusive( x, dps );
			for( int y = yrange.x; y <= yrange.y; y++ )
			{
				int2 zrange = context.zRangeInclusive( x, y, dps, six );
				for( int z = zrange.x; z <= zrange.y; z++ )
				{
					if( !context.intersect( context.p( x, y, z, dps ) ) ) continue;
					if( mortonOut && n < capacity )
					{
						int3 c = context.i( x, y, z );
						mortonOut[n] = encode2mortonCode_magicbits( c.x, c.y, c.z );
					}
					n++;
				}
			}
		}
		if( countsOut ) countsOut[t] = (uint32_t)( n - before );
	}
	return n;
}

// buildOctreeDAGReference (dag != 0) or buildOctreeNaive, then embedMask on every node (IntersectorOctree::embedMasks' loop) if embed != 0.
// nodesOut: 68-byte nodes, null to count.  buildOctreeNaive leaves nVoxelsPSum unwritten where a child is absent: compare mask and children only.
SHIM_API int64_t refw_build_octree( const uint64_t* mortonVoxels, int64_t nVoxels, int wide, int dag, int embed, OctreeNode* nodesOut, int64_t capacityNodes )
{
	std::vector<uint64_t> voxels( mortonVoxels, mortonVoxels + nVoxels );
	std::vector<OctreeNode> nodes;
	if( dag )
		buildOctreeDAGReference( &nodes, voxels, wide );
	else
		buildOctreeNaive( &nodes, voxels, wide );
	if( embed )
	{
		for( uint32_t i = 0; i < (uint32_t)nodes.size(); i++ ) embedMask( nodes.data(), i );
	}
	if( nodesOut )
	{
		std::copy( nodes.begin(), nodes.begin() + std::min<int64_t>( capacityNodes, (int64_t)nodes.size() ), nodesOut );
	}
	return (int64_t)nodes.size();
}

// Batch of IntersectorOctree::intersect (IntersectorOctree.hpp:248-257): root = last node, StackElement stack[32].  The traversal writes
// nothing on a miss, so the outputs are preset to what the oracle's callers preset: t = MAX_FLOAT, nMajor = -1, vIndex = 0.
SHIM_API void refw_trace_batch( const OctreeNode* nodes, int64_t nNodes, const float* lower3, const float* upper3, int64_t n, const float* ro, const float* rd,
								const uint8_t* isShadow, float* tOut, int32_t* nMajorOut, uint32_t* vIndexOut )
{
	const float3 lower = { lower3[0], lower3[1], lower3[2] };
	const float3 upper = { upper3[0], upper3[1], upper3[2] };
	StackElement stack[32];
	for( int64_t i = 0; i < n; i++ )
	{
		float t = MAX_FLOAT;
		int nMajor = -1;
		uint32_t vIndex = 0;
		octreeTraverse_EfficientParametric( nodes, (uint32_t)( nNodes - 1 ), stack, float3{ ro[i * 3], ro[i * 3 + 1], ro[i * 3 + 2] },
											float3{ rd[i * 3], rd[i * 3 + 1], rd[i * 3 + 2] }, lower, upper, &t, &nMajor, &vIndex, isShadow ? isShadow[i] != 0 : false );
		tOut[i] = t;
		nMajorOut[i] = nMajor;
		vIndexOut[i] = vIndex;
	}
}

SHIM_API void refw_get_hit_n( int major, const float* rd3, float* out3 )
{
	float3 n = getHitN<float3>( major, float3{ rd3[0], rd3[1], rd3[2] } );
	out3[0] = n.x;
	out3[1] = n.y;
	out3[2] = n.z;
}
SHIM_API int refw_bsearch_i32( const int* xs, int n, int x ) { return bSearch<int>( xs, n, x ); }
SHIM_API int refw_sort_bits_morton( uint32_t gridRes ) { return numberOfSortBitsMorton( gridRes ); }
SHIM_API uint32_t refw_hash_combine2( uint32_t a, uint32_t b ) { return hashCombine( a, b ); }
SHIM_API uint32_t refw_hash_combine3( uint32_t a, uint32_t b, uint32_t c ) { return hashCombine( a, b, c ); }
SHIM_API uint32_t refw_hash_combine4( uint32_t a, uint32_t b, uint32_t c, uint32_t d ) { return hashCombine( a, b, c, d ); }
