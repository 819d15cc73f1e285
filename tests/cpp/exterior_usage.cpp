// Compile-check of the exterior-mask and masked-extraction methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): the exterior masks of a hollow
// cube, and quads, welded mesh and merged rectangles from them.  Built and run by tests/test_gpu_exterior_app.py; run on a GPU with the argument `run`.
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // needs a GPU
	{
		std::printf( "usage: exterior_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// the shell of a 4 x 4 x 4 cube at (2, 2, 2) in a 16^3 grid: 56 voxels around 8 enclosed cells.  96 faces outside, 24 inside
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t z = 0; z < 4; z++ )
		for( uint32_t y = 0; y < 4; y++ )
			for( uint32_t x = 0; x < 4; x++ )
				if( x % 3 == 0 || y % 3 == 0 || z % 3 == 0 ) xyz.insert( xyz.end(), { 2 + x, 2 + y, 2 + z } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	std::vector<uint8_t> plain, masks;
	const uint64_t nPlain = svo.surfaceMasks( plain, stream );
	uint64_t nHidden = 7, hiddenOnly = 7;
	const uint64_t nExterior = svo.surfaceExteriorMasks( masks, &nHidden, stream );
	const uint64_t countOnly = svo.surfaceExteriorMasks( (uint8_t*)nullptr, &hiddenOnly, stream );
	std::vector<uint32_t> faceVoxel, meshVoxel, indices, rectVoxel, rectIndices, rectSize;
	std::vector<uint8_t> faceDir, meshDir, rectDir;
	std::vector<float> positions, vertices, rectVertices;
	svo.surfaceQuadsMasked( masks, faceVoxel, faceDir, positions, stream );
	svo.surfaceMeshMasked( masks, vertices, indices, meshVoxel, meshDir, stream );
	const uint64_t covered = svo.surfaceMergedMasked( masks, MVRT_SURFACE_MERGE_WELD, rectVertices, rectIndices, rectVoxel, rectDir, rectSize, stream );
	std::printf( "voxels %u plain %llu exterior %llu hidden %llu counts %llu %llu quads %zu mesh %zu vertices %zu covered %llu rects %zu corners %zu same %d\n", svo.m_numberOfVoxels,
				 (unsigned long long)nPlain, (unsigned long long)nExterior, (unsigned long long)nHidden, (unsigned long long)countOnly, (unsigned long long)hiddenOnly, faceVoxel.size(),
				 indices.size() / 4, vertices.size() / 3, (unsigned long long)covered, rectVoxel.size(), rectVertices.size() / 3, (int)( faceVoxel == meshVoxel && faceDir == meshDir ) );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return nPlain == 120 && nExterior == 96 && nHidden == 24 && countOnly == 96 && hiddenOnly == 24 && faceVoxel.size() == 96 && positions.size() == 96 * 12 && indices.size() == 96 * 4 &&
				   vertices.size() == 98 * 3 && covered == 96 && rectVoxel.size() == 6 && rectVertices.size() == 8 * 3 && faceVoxel == meshVoxel
			   ? 0
			   : 1;
}
