// Compile-check of the component methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp) and of the signatures of the two C calls: a hollow cube with
// debris around it is listed, then cleaned in place.  Built by tests/test_components_mirror.py; run on a GPU with the argument `run`.
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

static_assert( std::is_same<decltype( &mvrt_svo_components ),
							int ( * )( const mvrt_svo*, int, uint32_t*, uint64_t, uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_components" );
static_assert( std::is_same<decltype( &mvrt_svo_keep_components ), int ( * )( mvrt_svo*, int, uint64_t, uint32_t, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_keep_components" );

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: components_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// the one-voxel-thick shell of [4, 11)^3 in a 16^3 grid, 218 voxels, a speck at (1, 1, 1) and two voxels that touch at a corner
	std::vector<uint32_t> xyz = { 1, 1, 1, 13, 13, 13, 14, 14, 14 }, attribs;
	for( uint32_t z = 4; z < 11; z++ )
		for( uint32_t y = 4; y < 11; y++ )
			for( uint32_t x = 4; x < 11; x++ )
				if( !( x > 4 && x < 10 && y > 4 && y < 10 && z > 4 && z < 10 ) ) xyz.insert( xyz.end(), { x, y, z } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	const uint32_t all = svo.m_numberOfVoxels;
	uint64_t largest = 0;
	const uint64_t faces = svo.components( MVRT_MORPH_FACES, nullptr, 0, nullptr, nullptr, nullptr, &largest, stream ); // the sizing call
	std::vector<uint32_t> label, size, first, box;
	svo.components( MVRT_MORPH_CUBE, label, size, first, box, stream );
	const bool listed = label.size() == all && size.size() == 3 && first.size() == 3 && box.size() == 18 && size[0] == 1 && size[1] == 218 && size[2] == 2 && first[0] == 0 &&
						box[6] == 4 && box[9] == 10 && *std::max_element( label.begin(), label.end() ) == 2;
	uint64_t kept = 0;
	const uint64_t specks = svo.keepComponents( MVRT_MORPH_CUBE, 2, 0, &kept, stream ); // the single voxel goes
	const uint64_t debris = svo.keepComponents( MVRT_MORPH_CUBE, 1, 1, nullptr, stream ); // and everything but the shell
	const uint64_t none = svo.keepComponents();									 // nothing to drop: the octree is not touched
	std::printf( "voxels %u faces %llu largest %llu cube %zu listed %d specks %llu kept %llu debris %llu none %llu left %u\n", all, (unsigned long long)faces,
				 (unsigned long long)largest, size.size(), (int)listed, (unsigned long long)specks, (unsigned long long)kept, (unsigned long long)debris, (unsigned long long)none,
				 svo.m_numberOfVoxels );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return all == 221 && faces == 4 && largest == 218 && listed && specks == 1 && kept == 2 && debris == 2 && none == 0 && svo.m_numberOfVoxels == 218 ? 0 : 1;
}
