// Compile-check of the surface methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp): build an octree from a voxel list and extract its exposed
// faces as masks, quads and a welded mesh, through the host-vector forms and one device-pointer form.  Built by tests/test_surface_cpu.py; run on a GPU
// with the argument `run` (tests/test_gpu_surface.py).
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: surface_usage run\n" );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// a 2 x 2 x 2 block of voxels in a 16^3 grid: 24 exposed faces over 26 corner points
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t k = 0; k < 8; k++ ) xyz.insert( xyz.end(), { 4 + ( k & 1 ), 4 + ( ( k >> 1 ) & 1 ), 4 + ( k >> 2 ) } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );

	std::vector<uint8_t> masks, faceDir, meshDir;
	std::vector<uint32_t> faceVoxel, indices, meshVoxel;
	std::vector<float> positions, vertices;
	const uint64_t nFaces = svo.surfaceMasks( masks, stream );
	svo.surfaceQuads( faceVoxel, faceDir, positions, stream );
	svo.surfaceMesh( vertices, indices, meshVoxel, meshDir, stream );
	const uint64_t counted = svo.surfaceMasks( (uint8_t*)nullptr, stream ); // device-pointer form, count only
	bool same = faceVoxel == meshVoxel && faceDir == meshDir;
	for( size_t c = 0; c < indices.size() && same; c++ ) // a welded corner is the quad's corner, bit for bit
		for( int a = 0; a < 3; a++ ) same = vertices[(size_t)indices[c] * 3 + a] == positions[c * 3 + a];
	std::printf( "voxels %u masks %zu first %u faces %llu counted %llu quads %zu vertices %zu indices %zu same %d\n", svo.m_numberOfVoxels, masks.size(), masks[0],
				 (unsigned long long)nFaces, (unsigned long long)counted, faceVoxel.size(), vertices.size() / 3, indices.size(), same ? 1 : 0 );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return nFaces == 24 && counted == 24 && faceVoxel.size() == 24 && vertices.size() == 26 * 3 && same ? 0 : 1;
}
