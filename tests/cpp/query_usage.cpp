// Compile-check of the nearest-voxel query methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp) and of the signatures of the four C calls; without an
// argument it checks the refusals that need no GPU.  With the argument `run` (on a GPU) a coloured cube shell is queried at every cell of its grid and at a ring of
// outside points, compared with a second, shifted shell, and recoloured from it.  Built by tests/test_query_mirror.py, which compares every printed line with the
// Python wrapper and the model.
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

static_assert( std::is_same<decltype( &mvrt_svo_nearest_voxels ), int ( * )( const mvrt_svo*, uint64_t, const int32_t*, uint64_t, uint64_t*, uint32_t*, uint32_t*, void* )>::value,
			   "mvrt_svo_nearest_voxels" );
static_assert( std::is_same<decltype( &mvrt_svo_nearest_between ), int ( * )( const mvrt_svo*, const mvrt_svo*, const int32_t*, uint64_t, uint64_t, uint64_t*, uint32_t*, uint64_t*,
																				 uint64_t*, uint32_t*, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_nearest_between" );
static_assert( std::is_same<decltype( &mvrt_svo_transfer_attributes ), int ( * )( mvrt_svo*, const mvrt_svo*, const int32_t*, uint64_t, uint32_t, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_transfer_attributes" );
static_assert( std::is_same<decltype( &mvrt_test_nearest_query_stats ), int ( * )( uint64_t* )>::value, "mvrt_test_nearest_query_stats" );
static_assert( MVRT_TRANSFER_COLOUR == 1u && MVRT_TRANSFER_EMISSION == 2u && mvrt::IntersectorOctreeGPU::NO_LIMIT == UINT64_MAX, "the constants of the header" );

static int expectRefusal( int rc, const char* words, const char* what )
{
	const char* e = mvrt_last_error();
	if( rc != 0 && e && std::strstr( e, words ) ) return 0;
	std::printf( "FAILED %s: rc %d, error \"%s\", wanted \"%s\"\n", what, rc, e ? e : "", words );
	return 1;
}

// the shell of a 7^3 cube at (o, o, o), coloured by position, its x = o face emissive
static void shell( uint32_t o, uint32_t tint, std::vector<uint32_t>& xyz, std::vector<uint32_t>& colour )
{
	for( uint32_t z = 0; z < 7; z++ )
		for( uint32_t y = 0; y < 7; y++ )
			for( uint32_t x = 0; x < 7; x++ )
				if( x % 6 == 0 || y % 6 == 0 || z % 6 == 0 )
				{
					xyz.insert( xyz.end(), { o + x, o + y, o + z } );
					colour.insert( colour.end(), { 0x00000021u * x + 0x00002000u * y + 0x00200000u * z + tint, x == 0 ? 0x00000700u : 0u } );
				}
}

int main( int argc, char** argv )
{
	if( argc < 2 ) // the refusals the host makes before any GPU work
	{
		int bad = 0;
		mvrt_svo* h = nullptr;
		mvrt::check( mvrt_svo_create( &h ), "create" );
		uint64_t n = 7, stats[4];
		bad += expectRefusal( mvrt_svo_nearest_voxels( nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr ), "mvrt_svo_nearest_voxels: null handle", "query, null handle" );
		bad += expectRefusal( mvrt_svo_nearest_voxels( h, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr ), "mvrt_svo_nearest_voxels: no octree", "query, empty handle" );
		bad += expectRefusal( mvrt_svo_nearest_between( nullptr, h, nullptr, 0, 0, nullptr, nullptr, &n, nullptr, nullptr, nullptr, nullptr, nullptr ), "mvrt_svo_nearest_between: null handle",
							  "between, null handle" );
		bad += expectRefusal( mvrt_svo_nearest_between( h, h, nullptr, 0, 0, nullptr, nullptr, &n, nullptr, nullptr, nullptr, nullptr, nullptr ), "mvrt_svo_nearest_between: no octree",
							  "between, empty handle" );
		bad += n == 0 ? 0 : 1;
		bad += expectRefusal( mvrt_svo_transfer_attributes( nullptr, h, nullptr, 0, 3u, &n, nullptr, nullptr ), "mvrt_svo_transfer_attributes: null handle", "transfer, null handle" );
		bad += expectRefusal( mvrt_svo_transfer_attributes( h, h, nullptr, 0, 3u, &n, nullptr, nullptr ), "mvrt_svo_transfer_attributes: no octree", "transfer, empty handle" );
		bad += expectRefusal( mvrt_test_nearest_query_stats( nullptr ), "null out", "stats, null out" );
		bad += mvrt_test_nearest_query_stats( stats ) == 0 ? 0 : 1;
		mvrt_svo_destroy( h );
		std::printf( "usage: query_usage run (%d host checks failed)\n", bad );
		return bad;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU a, b;
	std::vector<uint32_t> xyz, colour;
	shell( 4, 0u, xyz, colour );
	a.buildFromVoxels( xyz, colour, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	xyz.clear(), colour.clear();
	shell( 6, 0x00010101u, xyz, colour );
	b.buildFromVoxels( xyz, colour, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	// every cell of the grid and a ring of points outside it
	std::vector<int32_t> query;
	for( int32_t z = 0; z < 16; z++ )
		for( int32_t y = 0; y < 16; y++ )
			for( int32_t x = 0; x < 16; x++ ) query.insert( query.end(), { x, y, z } );
	for( int32_t x : { -9, 3, 24 } )
		for( int32_t y : { -1, 16 } )
			for( int32_t z : { -17, 40 } ) query.insert( query.end(), { x, y, z } );
	std::vector<uint64_t> dist2;
	std::vector<uint32_t> nearest, attribs;
	a.nearestVoxels( query, mvrt::IntersectorOctreeGPU::NO_LIMIT, dist2, nearest, attribs, stream );
	unsigned long long sum = 0;
	for( size_t i = 0; i < dist2.size(); i++ ) sum += ( i + 1 ) * ( dist2[i] + 4913ull * nearest[i] ) + attribs[2 * i] + 3ull * attribs[2 * i + 1];
	std::printf( "queries %zu checksum %llu\n", dist2.size(), sum );
	a.nearestVoxels( query, 9, dist2, nearest, attribs, stream );
	sum = 0;
	for( size_t i = 0; i < dist2.size(); i++ ) sum += ( i + 1 ) * ( dist2[i] + 4913ull * nearest[i] ) + attribs[2 * i] + 3ull * attribs[2 * i + 1];
	std::printf( "limit 9 checksum %llu\n", sum );
	const int32_t offset[3] = { 1, 0, -1 };
	const mvrt::IntersectorOctreeGPU::Between r = a.nearestBetween( b, offset, mvrt::IntersectorOctreeGPU::NO_LIMIT, dist2, nearest, stream );
	const mvrt::IntersectorOctreeGPU::Between s = a.nearestBetween( b, offset, 4, 0, nullptr, nullptr, stream );
	sum = 0;
	for( size_t i = 0; i < dist2.size(); i++ ) sum += ( i + 1 ) * ( dist2[i] + 4913ull * nearest[i] );
	std::printf( "between n %llu max %llu farthest %u zero %llu beyond %llu checksum %llu; limit 4: max %llu farthest %u beyond %llu\n", (unsigned long long)r.n,
				 (unsigned long long)r.maxDist2, r.farthest, (unsigned long long)r.nZero, (unsigned long long)r.nBeyond, sum, (unsigned long long)s.maxDist2, s.farthest,
				 (unsigned long long)s.nBeyond );
	uint64_t beyond = 0;
	const uint64_t changed = a.transferAttributes( b, offset, 4, mvrt::IntersectorOctreeGPU::TRANSFER_COLOUR, &beyond, stream );
	const uint64_t again = a.transferAttributes( b, offset, 4, mvrt::IntersectorOctreeGPU::TRANSFER_COLOUR, nullptr, stream );
	std::vector<uint32_t> vx, va;
	a.readVoxels( vx, va, stream );
	sum = 0;
	for( size_t i = 0; i < va.size() / 2; i++ ) sum += ( i + 1 ) * ( va[2 * i] + 3ull * va[2 * i + 1] );
	std::printf( "transfer changed %llu beyond %llu again %llu emission %u checksum %llu\n", (unsigned long long)changed, (unsigned long long)beyond, (unsigned long long)again,
				 (unsigned)a.hasEmission(), sum );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return r.n == dist2.size() && again == 0 ? 0 : 1;
}
