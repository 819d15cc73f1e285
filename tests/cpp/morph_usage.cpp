// Compile-check of the morphology methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): a hollow cube with a one-voxel hole, which the fill finds
// empty of enclosed cells, is listed, closed, dilated, opened and eroded.  Built by tests/test_morph_mirror.py; run on a GPU with the argument `run`.
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: morph_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// the one-voxel-thick shell of [4, 11)^3 in a 16^3 grid without the voxel (7, 7, 10): 217 voxels
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t z = 4; z < 11; z++ )
		for( uint32_t y = 4; y < 11; y++ )
			for( uint32_t x = 4; x < 11; x++ )
			{
				const bool inner = x > 4 && x < 10 && y > 4 && y < 10 && z > 4 && z < 10;
				if( !inner && !( x == 7 && y == 7 && z == 10 ) ) xyz.insert( xyz.end(), { x, y, z } );
			}
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	const uint32_t shell = svo.m_numberOfVoxels;
	const uint64_t leaky = svo.enclosedCells( 0, nullptr, nullptr, nullptr, stream );
	std::vector<uint32_t> cells, cellAttribs, count, peeled;
	svo.dilationCells( MVRT_MORPH_CUBE, cells, cellAttribs, count, stream );
	svo.erosionVoxels( MVRT_MORPH_FACES, peeled, stream );
	const uint64_t plugged = svo.close( MVRT_MORPH_CUBE, 1, stream ); // exactly the hole
	const uint64_t enclosed = svo.enclosedCells( 0, nullptr, nullptr, nullptr, stream );
	const uint64_t grown = svo.dilate( MVRT_MORPH_FACES, 1, stream );
	const uint64_t opened = svo.open(); // nothing to remove: the octree is not touched
	const uint64_t eroded = svo.erode( MVRT_MORPH_FACES, 1, stream );
	std::printf( "shell %u leaky %llu cells %zu peeled %zu plugged %llu enclosed %llu grown %llu opened %llu eroded %llu left %u\n", shell, (unsigned long long)leaky, count.size(),
				 peeled.size(), (unsigned long long)plugged, (unsigned long long)enclosed, (unsigned long long)grown, (unsigned long long)opened, (unsigned long long)eroded,
				 svo.m_numberOfVoxels );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return shell == 217 && leaky == 0 && count.size() == 485 && peeled.size() == 217 && plugged == 1 && enclosed == 125 && grown == 392 && opened == 0 && eroded == 348 &&
				   svo.m_numberOfVoxels == 262
			   ? 0
			   : 1;
}
