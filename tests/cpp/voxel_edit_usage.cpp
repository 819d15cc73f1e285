// Compile-check of the voxel-list methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): build an octree from a voxel list, edit it,
// read it back.  Built by tests/test_voxel_edit_cpu.py; run on a GPU with the argument `run`.
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: voxel_edit_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// a 2 x 2 x 2 block of white voxels in a 16^3 grid, one of them listed twice
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t i = 0; i < 9; i++ )
	{
		const uint32_t k = i % 8;
		xyz.insert( xyz.end(), { 4 + ( k & 1 ), 4 + ( ( k >> 1 ) & 1 ), 4 + ( k >> 2 ) } );
	}
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	// paint one voxel red and emissive, remove another, add a new one
	const std::vector<uint32_t> exyz = { 4, 4, 4, 5, 5, 5, 0, 0, 0 };
	const std::vector<uint32_t> eattr = { 0xFF0000FFu, 0xFF0000FFu, 0, 0, 0xFF00FF00u, 0 };
	const std::vector<uint8_t> ops = { MVRT_VOXEL_SET, MVRT_VOXEL_REMOVE, MVRT_VOXEL_SET };
	svo.editVoxels( exyz, eattr, ops, stream );
	std::vector<uint32_t> gotXyz, gotAttribs;
	svo.readVoxels( gotXyz, gotAttribs, stream );
	std::printf( "voxels %u nodes %u hasEmission %u first (%u %u %u)\n", svo.m_numberOfVoxels, svo.m_numberOfNodes, svo.m_hasEmission, gotXyz[0], gotXyz[1], gotXyz[2] );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return svo.m_numberOfVoxels == 8 && svo.m_hasEmission == 1 && gotXyz[0] == 0 ? 0 : 1;
}
