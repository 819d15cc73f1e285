// Compile-check of the enclosed-cell methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): list the enclosed cells of a hollow cube, fill them,
// list again.  Built by tests/test_fill_cpu.py; run on a GPU with the argument `run`.
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: fill_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// the shell of a 4 x 4 x 4 cube at (2, 2, 2) in a 16^3 grid: 56 voxels around 8 enclosed cells
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t z = 0; z < 4; z++ )
		for( uint32_t y = 0; y < 4; y++ )
			for( uint32_t x = 0; x < 4; x++ )
				if( x % 3 == 0 || y % 3 == 0 || z % 3 == 0 ) xyz.insert( xyz.end(), { 2 + x, 2 + y, 2 + z } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	std::vector<uint32_t> cells, region;
	const uint64_t nRegions = svo.enclosedCells( cells, region, stream );
	const uint32_t before = svo.m_numberOfVoxels;
	const uint8_t red[8] = { 255, 0, 0, 255, 0, 0, 0, 255 };
	const uint64_t nFilled = svo.fillEnclosed( red, stream );
	const uint64_t again = svo.fillEnclosed( nullptr, stream );
	uint64_t regionsAfter = 7;
	const uint64_t cellsAfter = svo.enclosedCells( 0, nullptr, nullptr, &regionsAfter, stream );
	std::printf( "voxels %u cells %zu regions %llu first (%u %u %u) filled %llu voxels %u again %llu cells %llu regions %llu\n", before, region.size(), (unsigned long long)nRegions,
				 cells[0], cells[1], cells[2], (unsigned long long)nFilled, svo.m_numberOfVoxels, (unsigned long long)again, (unsigned long long)cellsAfter,
				 (unsigned long long)regionsAfter );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return before == 56 && region.size() == 8 && nRegions == 1 && nFilled == 8 && svo.m_numberOfVoxels == 64 && again == 0 && cellsAfter == 0 && regionsAfter == 0 ? 0 : 1;
}
