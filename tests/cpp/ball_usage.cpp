// Compile-check of the round-offset methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): the hollow cube with a one-voxel hole of morph_usage.cpp
// is measured, closed with the ball of 3, dilated, opened and eroded.  Built by tests/test_ball_mirror.py; run on a GPU with the argument `run`.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: ball_usage run\n" );
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
	std::vector<uint32_t> cells, dist2, nearest, cellAttribs, thin, depth2;
	svo.distanceCells( 3, cells, dist2, nearest, cellAttribs, stream ); // as a set, the cells of one CUBE step
	svo.depthVoxels( 1024, thin, depth2, stream );						  // every voxel of a one-voxel shell is 1 deep
	const uint32_t deepest = depth2.empty() ? 0u : *std::max_element( depth2.begin(), depth2.end() );
	const uint32_t farthest = dist2.empty() ? 0u : *std::max_element( dist2.begin(), dist2.end() );
	const uint64_t plugged = svo.closeBall( 3, stream ); // exactly the hole
	const uint64_t enclosed = svo.enclosedCells( 0, nullptr, nullptr, nullptr, stream );
	const uint64_t grown = svo.dilateBall( 1, stream );
	const uint64_t opened = svo.openBall( 3 ); // nothing to remove: the octree is not touched
	const uint64_t eroded = svo.erodeBall( 1, stream );
	std::printf( "shell %u cells %zu farthest %u thin %zu deepest %u plugged %llu enclosed %llu grown %llu opened %llu eroded %llu left %u\n", shell, dist2.size(), farthest,
				 thin.size(), deepest, (unsigned long long)plugged, (unsigned long long)enclosed, (unsigned long long)grown, (unsigned long long)opened, (unsigned long long)eroded,
				 svo.m_numberOfVoxels );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return shell == 217 && dist2.size() == 485 && farthest == 3 && thin.size() == 217 && deepest == 1 && plugged == 1 && enclosed == 125 && grown == 392 && opened == 0 &&
				   eroded == 348 && svo.m_numberOfVoxels == 262
			   ? 0
			   : 1;
}
