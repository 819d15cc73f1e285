// Compile-check of the distance-limit and occlusion methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp).  Built by tests/test_range_cpu.py; the
// direction table needs no GPU and is printed without arguments, the rest runs on a GPU with the argument `run`.
#include <cstdio>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

int main( int argc, char** argv )
{
	const std::vector<float> dirs = mvrt::IntersectorOctreeGPU::aoDirections( 4 ); // host only
	std::printf( "usage: range_usage run (directions %zu, first %.9g %.9g %.9g)\n", dirs.size() / 3, dirs[0], dirs[1], dirs[2] );
	if( argc < 2 ) return dirs.size() == 72 ? 0 : 1; // the rest needs a GPU
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	mvrt::IntersectorOctreeGPU svo;
	// two voxels two cells apart on x in an 8^3 grid
	std::vector<uint32_t> xyz = { 2, 4, 4, 5, 4, 4 }, attribs;
	svo.buildFromVoxels( xyz, attribs, mvrt::vec3{ 0, 0, 0 }, 1.0f, 8, 0, stream );
	std::vector<uint32_t> faceVoxel;
	std::vector<uint8_t> faceDir;
	std::vector<uint16_t> nearOpen, farOpen;
	svo.surfaceAo( 64, 1.0f, faceVoxel, faceDir, nearOpen, stream );
	svo.surfaceAo( 64, MVRT_MAX_FLOAT, faceVoxel, faceDir, farOpen, stream );
	unsigned nearAll = 0, farLess = 0;
	for( size_t f = 0; f < nearOpen.size(); f++ )
	{
		nearAll += nearOpen[f] == 64;
		farLess += farOpen[f] < 64;
	}
	// one ray along +x from outside the grid: it hits the first voxel at t = 3 (limit 4) and nothing within t <= 2
	const float ray[6] = { -1.0f, 4.5f, 4.5f, 1.0f, 0.0625f, 0.03125f }, limits[2] = { 4.0f, 2.0f };
	float t[2] = { 0, 0 };
	void *in = nullptr, *lim = nullptr, *out = nullptr;
	mvrt::check( mvrt_malloc( &in, 12 * sizeof( float ) ), "malloc" );
	mvrt::check( mvrt_malloc( &lim, sizeof( limits ) ), "malloc" );
	mvrt::check( mvrt_malloc( &out, sizeof( t ) ), "malloc" );
	float soa[12];
	for( int k = 0; k < 6; k++ ) soa[2 * k] = soa[2 * k + 1] = ray[k];
	mvrt::check( mvrt_memcpy_h2d( in, soa, sizeof( soa ), stream ), "h2d" );
	mvrt::check( mvrt_memcpy_h2d( lim, limits, sizeof( limits ), stream ), "h2d" );
	const float* p = (const float*)in;
	svo.intersectRange( 2, p, p + 2, p + 4, p + 6, p + 8, p + 10, nullptr, (const float*)lim, (float*)out, nullptr, nullptr, nullptr, stream );
	mvrt::check( mvrt_memcpy_d2h( t, out, sizeof( t ), stream ), "d2h" );
	std::printf( "faces %zu nearAll %u farLess %u t %.9g %.9g\n", faceVoxel.size(), nearAll, farLess, t[0], t[1] );
	mvrt_free( in );
	mvrt_free( lim );
	mvrt_free( out );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return faceVoxel.size() == 12 && nearAll == 12 && farLess == 2 && t[0] == 3.0f && t[1] == MVRT_MAX_FLOAT ? 0 : 1;
}
