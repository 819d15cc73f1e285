// Compile-check of surfaceMerged of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): the full 2^3 grid merges into its six 2 x 2 sides over the eight
// corners of the cube, through the host-vector form with and without the weld flag and through the device-pointer form as the sizing call.  Built by
// tests/test_surface_merge_cpu.py; run on a GPU with the argument `run` (tests/test_gpu_surface_merge.py).
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: surface_merge_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t k = 0; k < 8; k++ ) xyz.insert( xyz.end(), { k & 1, ( k >> 1 ) & 1, k >> 2 } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 0.5f, 2, 0, stream );

	std::vector<float> vertices, corners;
	std::vector<uint32_t> indices, none, rectVoxel, rectSize, voxel2, size2;
	std::vector<uint8_t> rectDir, dir2;
	const uint64_t nFaces = svo.surfaceMerged( MVRT_SURFACE_MERGE_WELD, vertices, indices, rectVoxel, rectDir, rectSize, stream );
	const uint64_t nFaces2 = svo.surfaceMerged( 0, corners, none, voxel2, dir2, size2, stream );
	uint64_t nf = 0, nr = 0, nv = 0;
	svo.surfaceMerged( MVRT_SURFACE_MERGE_ANY_ATTRIBUTE | MVRT_SURFACE_MERGE_WELD, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nf, &nr, &nv, stream );
	bool same = rectVoxel == voxel2 && rectDir == dir2 && rectSize == size2 && none.empty() && corners.size() == indices.size() * 3;
	for( size_t c = 0; c < indices.size() && same; c++ ) // a welded corner is the rectangle's corner, bit for bit
		for( int a = 0; a < 3; a++ ) same = vertices[(size_t)indices[c] * 3 + a] == corners[c * 3 + a];
	bool twoByTwo = true;
	for( uint32_t s : rectSize ) twoByTwo = twoByTwo && s == 2;
	std::printf( "faces %llu rects %zu vertices %zu sized %llu %llu %llu same %d two %d\n", (unsigned long long)nFaces, rectVoxel.size(), vertices.size() / 3, (unsigned long long)nf,
				 (unsigned long long)nr, (unsigned long long)nv, same ? 1 : 0, twoByTwo ? 1 : 0 );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return nFaces == 24 && nFaces2 == 24 && rectVoxel.size() == 6 && vertices.size() == 8 * 3 && nf == 24 && nr == 6 && nv == 8 && same && twoByTwo ? 0 : 1;
}
