// Compile-check of the two-set methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp) and of the signatures of the two C calls: a 4^3 brush is listed
// against a hollow cube under every operator, at an offset that clips a part of it, then stamped in and carved out in place.  Built by
// tests/test_combine_mirror.py; run on a GPU with the argument `run`, where the same test compares every printed line with the Python wrapper.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

static_assert( std::is_same<decltype( &mvrt_svo_combine_voxels ), int ( * )( const mvrt_svo*, const mvrt_svo*, int, const int32_t*, uint32_t, uint64_t, uint32_t*, uint32_t*, uint8_t*,
																			 uint64_t*, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_combine_voxels" );
static_assert( std::is_same<decltype( &mvrt_svo_combine ),
							int ( * )( mvrt_svo*, const mvrt_svo*, int, const int32_t*, uint32_t, uint64_t*, uint64_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_combine" );
static_assert( mvrt::IntersectorOctreeGPU::COMBINE_UNION == 0 && mvrt::IntersectorOctreeGPU::COMBINE_INTERSECTION == 1 && mvrt::IntersectorOctreeGPU::COMBINE_DIFFERENCE == 2 &&
				   mvrt::IntersectorOctreeGPU::COMBINE_XOR == 3 && mvrt::IntersectorOctreeGPU::COMBINE_ATTRIB_B == 1,
			   "COMBINE_*" );

// what the Python side recomputes from its own listing: a sum over the voxels in which position, coordinates, both attribute words and the source byte count
static unsigned long long checksum( const std::vector<uint32_t>& xyz, const std::vector<uint32_t>& attribs, const std::vector<uint8_t>& source )
{
	unsigned long long s = 0;
	for( size_t i = 0; i < source.size(); i++ )
		s += ( i + 1 ) * ( xyz[3 * i] + 17ull * xyz[3 * i + 1] + 289ull * xyz[3 * i + 2] + 4913ull * source[i] ) + attribs[2 * i] + 3ull * attribs[2 * i + 1];
	return s;
}

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: combine_usage run\n" );
		return 0;
	}
	using Svo = mvrt::IntersectorOctreeGPU;
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	Svo cube, brush;
	// the one-voxel-thick shell of [2, 14)^3 in a 16^3 grid, 728 voxels, white; the full 4^3 grid in one colour with some emission
	std::vector<uint32_t> shell, none, block, colour;
	for( uint32_t z = 2; z < 14; z++ )
		for( uint32_t y = 2; y < 14; y++ )
			for( uint32_t x = 2; x < 14; x++ )
				if( !( x > 2 && x < 13 && y > 2 && y < 13 && z > 2 && z < 13 ) ) shell.insert( shell.end(), { x, y, z } );
	for( uint32_t z = 0; z < 4; z++ )
		for( uint32_t y = 0; y < 4; y++ )
			for( uint32_t x = 0; x < 4; x++ )
			{
				block.insert( block.end(), { x, y, z } );
				colour.insert( colour.end(), { 0x00302010u, 0x00000500u } );
			}
	cube.buildFromVoxels( shell, none, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	brush.buildFromVoxels( block, colour, mvrt::vec3{ 0, 0, 0 }, 1.0f / 4, 4, 0, stream );
	const int32_t offset[3] = { 9, 13, 8 }; // the brush's y = 13 lies in a face of the shell, its y = 16 leaves the grid
	for( int op = Svo::COMBINE_UNION; op <= Svo::COMBINE_XOR; op++ )
	{
		std::vector<uint32_t> xyz, attribs;
		std::vector<uint8_t> source;
		uint64_t overlap = 0, clipped = 0;
		cube.combineVoxels( brush, op, offset, Svo::COMBINE_ATTRIB_B, xyz, attribs, source, &overlap, &clipped, stream );
		const uint64_t sized = cube.combineVoxels( brush, op, offset, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, stream ); // the sizing call
		std::printf( "op %d n %zu sized %llu overlap %llu clipped %llu checksum %llu\n", op, source.size(), (unsigned long long)sized, (unsigned long long)overlap,
					 (unsigned long long)clipped, checksum( xyz, attribs, source ) );
	}
	uint64_t removed = 0, clipped = 0;
	const uint64_t added = cube.combine( brush, Svo::COMBINE_UNION, offset, 0, &removed, &clipped, stream );
	std::printf( "union added %llu removed %llu clipped %llu voxels %u emission %u\n", (unsigned long long)added, (unsigned long long)removed, (unsigned long long)clipped,
				 cube.m_numberOfVoxels, (unsigned)cube.hasEmission() );
	const uint64_t again = cube.combine( brush, Svo::COMBINE_UNION, offset ); // nothing to add: the octree is not touched
	uint64_t corner = 0;
	cube.combine( brush, Svo::COMBINE_DIFFERENCE, nullptr, 0, &corner ); // the brush where it stands, at the origin: a corner of the shell goes
	const int32_t back[3] = { 9, 12, 8 };
	cube.combine( brush, Svo::COMBINE_DIFFERENCE, back, 0, &removed, &clipped, stream );
	std::printf( "again %llu corner %llu carved %llu clipped %llu voxels %u emission %u\n", (unsigned long long)again, (unsigned long long)corner, (unsigned long long)removed,
				 (unsigned long long)clipped, cube.m_numberOfVoxels, (unsigned)cube.hasEmission() );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return again == 0 ? 0 : 1;
}
