// Compile-check (and, with "run", a GPU walk-through) of the luminance moments and the denoiser on the header-only C++ mirror:
// PathTracer::setMoments, PathTracer::denoise, m_momentsF32, m_denoisedF32 (include/mvrt/PathTracer.hpp).  Built by tests/test_denoise_cpu.py and
// tests/test_gpu_denoise.py.
#include <cstdio>
#include <vector>

#include "mvrt/PathTracer.hpp"

struct V3 // stand-in for glm::vec3
{
	float x, y, z;
};

int main( int argc, char** argv )
{
	mvrt_denoise_params params;
	mvrt::check( mvrt_denoise_default_params( &params ), "default_params" );
	if( argc < 2 ) // never goes further in the CPU test: the rest needs a GPU
	{
		std::printf( "usage: denoise_usage run (iterations %d structBytes %u scratch %llu)\n", params.iterations, params.structBytes, (unsigned long long)mvrt_denoise_scratch_bytes( 64, 36 ) );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	std::vector<V3> vertices = { { 0.1f, 0.1f, 0.1f }, { 0.9f, 0.2f, 0.3f }, { 0.4f, 0.8f, 0.7f } }, vcolors, vemissions;
	mvrt::PathTracer pt;
	pt.setup( stream );
	pt.setAOVs( true );
	pt.setMoments( true ); // before the frame exists: allocated by the resize
	pt.resizeFrameBufferIfNeeded( stream, 64, 36 );
	std::printf( "views %d %d bytes %lld\n", (int)( pt.m_momentsF32 != nullptr ), (int)( pt.m_denoisedF32 != nullptr ), (long long)pt.m_momentsF32->bytes() );
	pt.loadHDRI( stream, "monks_forest_s.hdr" );
	pt.updateScene( vertices, vcolors, vemissions, stream, V3{ 0, 0, 0 }, 1.0f / 64, 64 );
	const float view[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.5f, -0.5f, -3, 1 };
	const float proj[16] = { 1.3f, 0, 0, 0, 0, 2.4f, 0, 0, 0, 0, -1, -1, 0, 0, -0.2f, 0 };
	pt.clearFrameBuffer( stream );
	pt.step( stream, view, proj, 3.0f, 0.01f );
	pt.step( stream, view, proj, 3.0f, 0.01f );
	params.iterations = 3;
	pt.denoise( stream, &params );
	// a caller's own read of the view on the stream of the denoise == mvrt_pt_read_denoised
	std::vector<float> own( 64 * 36 * 4 ), viaRead( 64 * 36 * 4 );
	mvrt::check( mvrt_memcpy_d2h( own.data(), pt.m_denoisedF32->data(), own.size() * 4, stream ), "d2h" );
	mvrt::check( mvrt_stream_synchronize( stream ), "sync" );
	mvrt::check( mvrt_pt_read_denoised( pt.handle(), stream, viaRead.data() ), "read_denoised" );
	bool wOne = true;
	for( size_t i = 3; i < own.size(); i += 4 ) wOne = wOne && own[i] == 1.0f;
	std::printf( "denoised %d bytes %lld w %d same %d steps %d\n", (int)( pt.m_denoisedF32 != nullptr ), (long long)pt.m_denoisedF32->bytes(), (int)wOne, (int)( own == viaRead ), pt.getSteps() );
	// a call refused on the host (through the C entry: the mirror's check() aborts) leaves the image of the last call and its view in place
	params.iterations = 9;
	const int rc = mvrt_pt_denoise( pt.handle(), stream, &params );
	std::printf( "refused %d view %d\n", (int)( rc != 0 ), (int)( pt.m_denoisedF32->data() == (char*)mvrt_pt_denoised_dev( pt.handle() ) ) );
	pt.denoise( stream );
	pt.resizeFrameBufferIfNeeded( stream, 32, 20 ); // the library releases the denoised image: no stale view survives
	std::printf( "resized %d\n", (int)( pt.m_denoisedF32 == nullptr && pt.m_momentsF32 != nullptr && pt.m_momentsF32->bytes() == 768 * 16 ) );
	pt.setMoments( false );
	std::printf( "off %d\n", (int)( pt.m_momentsF32 == nullptr && mvrt_pt_moments_dev( pt.handle() ) == nullptr ) );
	pt.setMoments( true );
	pt.setTile( 0, 2 );
	std::printf( "tile %d %d\n", (int)( pt.m_momentsF32 == nullptr ), (int)( pt.m_denoisedF32 == nullptr ) );
	pt.cleanUp();
	return 0;
}
