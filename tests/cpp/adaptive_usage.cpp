// Compile-check (and, with "run", a GPU walk-through) of adaptive sampling on the header-only C++ mirror: PathTracer::setSampleMask, PathTracer::activePixels,
// PathTracer::errorMask (include/mvrt/PathTracer.hpp).  Built by tests/test_adaptive_cpu.py and tests/test_gpu_adaptive.py.
#include <cstdio>
#include <vector>

#include "mvrt/PathTracer.hpp"

struct V3 // stand-in for glm::vec3
{
	float x, y, z;
};

int main( int argc, char** argv )
{
	if( argc < 2 ) // never goes further in the CPU test: the rest needs a GPU.  Without a frame both calls are refused on the host
	{
		mvrt_pt* h = nullptr;
		mvrt::check( mvrt_pt_create( &h ), "create" );
		uint8_t dummy = 0;
		const int a = mvrt_pt_set_sample_mask( h, nullptr, &dummy, nullptr );
		const int b = mvrt_pt_error_mask( h, nullptr, 0.05f, 0.01f, 32, 0, &dummy, nullptr );
		std::printf( "usage: adaptive_usage run (refused %d %d active %llu)\n", (int)( a != 0 ), (int)( b != 0 ), (unsigned long long)mvrt_pt_active_pixels( h ) );
		mvrt_pt_destroy( h );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	std::vector<V3> vertices = { { 0.1f, 0.1f, 0.1f }, { 0.9f, 0.2f, 0.3f }, { 0.4f, 0.8f, 0.7f } }, vcolors, vemissions;
	mvrt::PathTracer pt;
	pt.setup( stream );
	pt.setMoments( true );
	pt.resizeFrameBufferIfNeeded( stream, 64, 36 );
	pt.loadHDRI( stream, "monks_forest_s.hdr" );
	pt.updateScene( vertices, vcolors, vemissions, stream, V3{ 0, 0, 0 }, 1.0f / 64, 64 );
	const float view[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.5f, -0.5f, -3, 1 };
	const float proj[16] = { 1.3f, 0, 0, 0, 0, 2.4f, 0, 0, 0, 0, -1, -1, 0, 0, -0.2f, 0 };
	const uint64_t owned = mvrt_pt_owned_pixels( pt.handle() ), pixels = 64 * 36;
	std::printf( "active %llu of %llu owned\n", (unsigned long long)pt.activePixels(), (unsigned long long)owned );
	pt.clearFrameBuffer( stream );
	pt.step( stream, view, proj, 3.0f, 0.01f );
	pt.step( stream, view, proj, 3.0f, 0.01f );
	uint8_t* maskDev = nullptr;
	mvrt::check( mvrt_malloc( (void**)&maskDev, owned ), "malloc" );
	// every pixel has 32 samples: with minSamples 48 all of them are marked, with maxSamples 32 none
	const uint64_t all = pt.errorMask( stream, 0.05f, maskDev, 0.01f, 48 ), none = pt.errorMask( stream, 0.05f, maskDev, 0.01f, 32, 32 );
	const uint64_t some = pt.errorMask( stream, 0.05f, maskDev );
	const uint64_t set = pt.setSampleMask( stream, maskDev );
	std::printf( "marked %llu %llu %llu set %llu active %llu\n", (unsigned long long)all, (unsigned long long)none, (unsigned long long)some, (unsigned long long)set,
				 (unsigned long long)pt.activePixels() );
	pt.step( stream, view, proj, 3.0f, 0.01f );
	std::vector<float> fb( owned * 4 );
	std::vector<uint8_t> mask( owned );
	mvrt::check( mvrt_pt_read_framebuffer( pt.handle(), stream, fb.data() ), "read_framebuffer" );
	mvrt::check( mvrt_memcpy_d2h( mask.data(), maskDev, owned, stream ), "d2h" );
	mvrt::check( mvrt_stream_synchronize( stream ), "sync" );
	bool counts = true;
	for( uint64_t p = 0; p < pixels; p++ ) counts = counts && fb[p * 4 + 3] == ( mask[p] ? 48.0f : 32.0f );
	std::printf( "counts %d steps %d\n", (int)counts, pt.getSteps() );
	std::printf( "off %llu\n", (unsigned long long)pt.setSampleMask( stream, nullptr ) );
	pt.setSampleMask( stream, maskDev );
	pt.clearFrameBuffer( stream ); // a new frame needs every pixel
	std::printf( "cleared %llu\n", (unsigned long long)pt.activePixels() );
	mvrt_free( maskDev );
	pt.cleanUp();
	return 0;
}
