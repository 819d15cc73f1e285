// Compile-check of the nearest-voxel methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp) and of the signatures of the three C calls; without an
// argument it checks the refusals that need no GPU.  With the argument `run` (on a GPU) the enclosed cells of a coloured shell with one floating voxel are listed
// with their nearest voxel and then filled.  Built by tests/test_nearest_mirror.py, which compares every printed line with the Python wrapper and the model.
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

static_assert( std::is_same<decltype( &mvrt_svo_enclosed_nearest ),
							int ( * )( const mvrt_svo*, uint64_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_enclosed_nearest" );
static_assert( std::is_same<decltype( &mvrt_svo_fill_enclosed_nearest ), int ( * )( mvrt_svo*, uint64_t*, void* )>::value, "mvrt_svo_fill_enclosed_nearest" );
static_assert( std::is_same<decltype( &mvrt_test_enclosed_nearest_stats ), int ( * )( uint64_t* )>::value, "mvrt_test_enclosed_nearest_stats" );

static int expectRefusal( int rc, const char* words, const char* what )
{
	const char* e = mvrt_last_error();
	if( rc != 0 && e && std::strstr( e, words ) ) return 0;
	std::printf( "FAILED %s: rc %d, error \"%s\", wanted \"%s\"\n", what, rc, e ? e : "", words );
	return 1;
}

int main( int argc, char** argv )
{
	if( argc < 2 ) // the refusals the host makes before any GPU work
	{
		int bad = 0;
		mvrt_svo* h = nullptr;
		mvrt::check( mvrt_svo_create( &h ), "create" );
		uint64_t n = 7, r = 7, stats[8];
		bad += expectRefusal( mvrt_svo_enclosed_nearest( nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n, &r, nullptr ), "mvrt_svo_enclosed_nearest: null handle", "listing, null handle" );
		bad += expectRefusal( mvrt_svo_enclosed_nearest( h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n, &r, nullptr ), "mvrt_svo_enclosed_nearest: no octree", "listing, empty handle" );
		bad += expectRefusal( mvrt_svo_fill_enclosed_nearest( nullptr, &n, nullptr ), "mvrt_svo_fill_enclosed_nearest: null handle", "fill, null handle" );
		bad += expectRefusal( mvrt_svo_fill_enclosed_nearest( h, &n, nullptr ), "mvrt_svo_fill_enclosed_nearest: no octree", "fill, empty handle" );
		bad += expectRefusal( mvrt_test_enclosed_nearest_stats( nullptr ), "null out", "stats, null out" );
		bad += mvrt_test_enclosed_nearest_stats( stats ) == 0 ? 0 : 1;
		mvrt_svo_destroy( h );
		std::printf( "usage: nearest_usage run (%d host checks failed)\n", bad );
		return bad;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// the shell of a 7^3 cube at (2, 2, 2) in a 16^3 grid around 125 cells, coloured by position, its x = 2 face emissive, and one voxel floating inside
	std::vector<uint32_t> xyz, colour;
	for( uint32_t z = 0; z < 7; z++ )
		for( uint32_t y = 0; y < 7; y++ )
			for( uint32_t x = 0; x < 7; x++ )
				if( x % 6 == 0 || y % 6 == 0 || z % 6 == 0 || ( x == 2 && y == 4 && z == 3 ) )
				{
					xyz.insert( xyz.end(), { 2 + x, 2 + y, 2 + z } );
					colour.insert( colour.end(), { 0x00000021u * x + 0x00002000u * y + 0x00200000u * z, x == 0 ? 0x00000700u : 0u } );
				}
	svo.buildFromVoxels( xyz, colour, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	std::vector<uint32_t> cells, region, dist2, nearest, attribs;
	const uint64_t nRegions = svo.enclosedNearest( cells, region, dist2, nearest, attribs, stream );
	uint64_t sizedRegions = 0;
	const uint64_t sized = svo.enclosedNearest( 0, nullptr, nullptr, nullptr, nullptr, nullptr, &sizedRegions, stream );
	unsigned long long sum = 0;
	uint32_t deepest = 0;
	for( size_t i = 0; i < region.size(); i++ )
	{
		sum += ( i + 1 ) * ( cells[3 * i] + 17ull * cells[3 * i + 1] + 289ull * cells[3 * i + 2] + 4913ull * dist2[i] + 83521ull * nearest[i] + region[i] ) + attribs[2 * i] + 3ull * attribs[2 * i + 1];
		deepest = dist2[i] > deepest ? dist2[i] : deepest;
	}
	std::printf( "listing n %zu sized %llu regions %llu %llu deepest %u checksum %llu\n", region.size(), (unsigned long long)sized, (unsigned long long)nRegions,
				 (unsigned long long)sizedRegions, deepest, sum );
	const uint32_t before = svo.m_numberOfVoxels;
	const uint64_t nFilled = svo.fillEnclosedNearest( stream );
	const uint64_t again = svo.fillEnclosedNearest();
	std::printf( "fill voxels %u -> %u filled %llu again %llu emission %u\n", before, svo.m_numberOfVoxels, (unsigned long long)nFilled, (unsigned long long)again, (unsigned)svo.hasEmission() );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return sized == region.size() && nFilled == sized && again == 0 ? 0 : 1;
}
