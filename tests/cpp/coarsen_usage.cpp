// Compile-check of the level-of-detail methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): list the coarse voxels of a small block, coarsen it into
// a second object and in place.  Built by tests/test_coarsen_cpu.py; run on a GPU with the argument `run`.
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: coarsen_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo, lod;
	// a 4 x 4 x 4 block at (2, 2, 2) in a 16^3 grid and one stray voxel: at k = 1 the block covers 27 cells of 1 to 8 voxels, the stray voxel a cell of its own
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t z = 0; z < 4; z++ )
		for( uint32_t y = 0; y < 4; y++ )
			for( uint32_t x = 0; x < 4; x++ ) xyz.insert( xyz.end(), { 3 + x, 3 + y, 3 + z } );
	xyz.insert( xyz.end(), { 12u, 13u, 14u } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	std::vector<uint32_t> cells, cellAttribs, count;
	svo.coarseVoxels( 1, 1, cells, cellAttribs, count, stream );
	const uint64_t solid = svo.coarseVoxels( 1, 8, 0, nullptr, nullptr, nullptr, stream ); // the sizing call: only the one full cell
	svo.coarsen( 1, 2, MVRT_BUILD_NO_DAG, &lod, stream );										// drops the stray voxel and the block's corner cells
	const uint32_t fine = svo.m_numberOfVoxels, coarse = lod.m_numberOfVoxels;
	svo.coarsen( 2 ); // in place
	std::printf( "voxels %u cells %zu solid %llu lod %u in place %u\n", fine, count.size(), (unsigned long long)solid, coarse, svo.m_numberOfVoxels );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return fine == 65 && count.size() == 28 && solid == 1 && coarse == 19 && svo.m_numberOfVoxels == 9 ? 0 : 1;
}
