// Compile-check of the walk methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): upload a small octree written by hand, list its voxels with
// walkVoxels, make it a library-built octree with rebuild, then read the voxels back and take the exposure masks, which an upload alone refuses.  Built by
// tests/test_walk_cpu.py; run on a GPU with the argument `run` (tests/test_gpu_walk.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

struct Node68 // the reference's node: mask (+ 3 bytes padding), children[8], nVoxelsPSum[8]
{
	uint32_t mask, children[8], psum[8];
};
static_assert( sizeof( Node68 ) == 68, "reference node layout" );

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: walk_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	// a 4^3 grid, a DAG of two nodes: node 0 holds the voxels of slots 0 and 7 and is the root's child in slots 0 and 3 -> four voxels, codes 0, 7, 24, 31
	Node68 nodes[2];
	std::memset( nodes, 0xFF, sizeof( nodes ) );
	nodes[0].mask = 0x81u;
	nodes[1].mask = 0x09u;
	for( int c = 0; c < 8; c++ ) nodes[0].psum[c] = nodes[1].psum[c] = 0;
	nodes[0].psum[7] = 1;
	nodes[1].children[0] = nodes[1].children[3] = 0u | 0x81u << 24; // embedded: index | the child's mask
	nodes[1].psum[3] = 2;
	std::vector<uint32_t> attribsIn = { 0x10111213u, 0x00000000u, 0x20212223u, 0x7F000000u, 0x30313233u, 0x00000000u, 0x40414243u, 0x01020304u }; // alpha bytes are kept as they are
	mvrt::IntersectorOctreeGPU svo;
	svo.upload( nodes, 2, attribsIn.data(), 4, mvrt::vec3{ 0, 0, 0 }, 0.25f, 4, true, true, stream );

	std::vector<uint32_t> xyz, vIndex, attribs, xyzBack, attribsBack;
	svo.walkVoxels( xyz, vIndex, attribs, stream );
	const uint64_t counted = svo.walkVoxels( 0, nullptr, nullptr, nullptr, stream ); // device-pointer form, the sizing call
	const std::vector<uint32_t> wantXyz = { 0, 0, 0, 1, 1, 1, 2, 2, 0, 3, 3, 1 }, wantIndex = { 0, 1, 2, 3 };
	const bool walked = xyz == wantXyz && vIndex == wantIndex && attribs == attribsIn;

	svo.rebuild();
	svo.readVoxels( xyzBack, attribsBack, stream );
	std::vector<uint8_t> masks;
	const uint64_t nFaces = svo.surfaceMasks( masks, stream );
	const bool same = xyzBack == xyz && attribsBack == attribs;
	std::printf( "paths %zu counted %llu walked %d voxels %u emission %u same %d faces %llu\n", vIndex.size(), (unsigned long long)counted, walked ? 1 : 0, svo.m_numberOfVoxels,
				 svo.m_hasEmission, same ? 1 : 0, (unsigned long long)nFaces );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return walked && counted == 4 && same && svo.m_numberOfVoxels == 4 && nFaces == 24 ? 0 : 1;
}
