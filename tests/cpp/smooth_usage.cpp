// Compile-check of the smoothing methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp) and of the C signatures behind them (include/mvrt.h): the
// welded mesh of a 2 x 2 x 2 block smoothed with the defaults, without an iteration, on caller masks and through the device-pointer form.  Built by
// tests/test_smooth_mirror.py; run on a GPU with the argument `run` (tests/test_gpu_smooth_app.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

// the C signatures, pinned: a change of either declaration stops this file from compiling
static int ( *const pinDefaults )( mvrt_smooth_params* ) = mvrt_smooth_default_params;
static int ( *const pinSmooth )( const mvrt_svo*, const uint8_t*, const mvrt_smooth_params*, uint64_t, uint64_t, uint32_t*, uint8_t*, uint32_t*, float*, int32_t*, uint8_t*, uint64_t*, uint64_t*,
								 uint64_t*, void* ) = mvrt_svo_surface_smooth;
static_assert( sizeof( mvrt_smooth_params ) == 32 && MVRT_SMOOTH_STEPS_PER_CELL == 256, "mvrt_smooth_params: four int32 and four reserved words" );

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: smooth_usage run\n" );
		return 0;
	}
	mvrt_smooth_params viaPin;
	mvrt::check( pinDefaults( &viaPin ), "mvrt_smooth_default_params" );
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// a 2 x 2 x 2 block of voxels in a 16^3 grid: 24 exposed faces over 26 corner points
	std::vector<uint32_t> xyz, attribs;
	for( uint32_t k = 0; k < 8; k++ ) xyz.insert( xyz.end(), { 4 + ( k & 1 ), 4 + ( ( k >> 1 ) & 1 ), 4 + ( k >> 2 ) } );
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );

	std::vector<uint8_t> faceDir, plainDir, topDir;
	std::vector<uint32_t> indices, faceVoxel, plainIndices, plainVoxel, topIndices, topVoxel;
	std::vector<float> vertices, still, plain, top;
	mvrt_smooth_params p = mvrt::IntersectorOctreeGPU::smoothDefaultParams();
	const uint64_t clamped = svo.surfaceSmooth( p, vertices, indices, faceVoxel, faceDir, stream );
	svo.surfaceMesh( plain, plainIndices, plainVoxel, plainDir, stream );
	p.iterations = 0;
	const uint64_t none = svo.surfaceSmooth( p, still, indices, faceVoxel, faceDir, stream );
	const bool same = still == plain && indices == plainIndices && faceVoxel == plainVoxel && faceDir == plainDir; // no iteration: the plain mesh
	size_t moved = 0;
	for( size_t v = 0; v < plain.size() / 3; v++ ) moved += vertices[v * 3] != plain[v * 3] || vertices[v * 3 + 1] != plain[v * 3 + 1] || vertices[v * 3 + 2] != plain[v * 3 + 2];
	p.iterations = 4;
	const std::vector<uint8_t> masks( svo.m_numberOfVoxels, 2 ); // the +Y faces alone: an open sheet of 8 quads
	const uint64_t topClamped = svo.surfaceSmooth( masks, p, top, topIndices, topVoxel, topDir, stream );
	uint64_t nFaces = 0, nVertices = 0, sizingClamped = 7; // device-pointer form: the sizing call
	svo.surfaceSmooth( nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nFaces, &nVertices, &sizingClamped, stream );
	std::printf( "faces %llu vertices %llu clamped %llu moved %zu none %llu same %d top faces %zu vertices %zu clamped %llu sizing %llu\n", (unsigned long long)nFaces,
				 (unsigned long long)nVertices, (unsigned long long)clamped, moved, (unsigned long long)none, same ? 1 : 0, topVoxel.size(), top.size() / 3, (unsigned long long)topClamped,
				 (unsigned long long)sizingClamped );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return nFaces == 24 && nVertices == 26 && vertices.size() == 26 * 3 && same && none == 0 && sizingClamped == 0 ? 0 : 1;
}
