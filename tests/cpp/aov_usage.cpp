// Compile-check (and, with "run", a GPU walk-through) of the first-hit feature buffers on the header-only C++ mirror:
// PathTracer::setAOVs, m_aovAlbedoF32, m_aovNormalDepthF32 (include/mvrt/PathTracer.hpp).  Built by tests/test_aov_cpu.py.
#include <cstdio>
#include <vector>

#include "mvrt/PathTracer.hpp"

struct V3 // stand-in for glm::vec3
{
	float x, y, z;
};

int main( int argc, char** argv )
{
	if( argc < 2 ) // never executed by the CPU test: needs a GPU
	{
		std::printf( "usage: aov_usage run (MVRT_AOV_ALBEDO %d MVRT_AOV_NORMAL_DEPTH %d)\n", MVRT_AOV_ALBEDO, MVRT_AOV_NORMAL_DEPTH );
		return 0;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	std::vector<V3> vertices = { { 0.1f, 0.1f, 0.1f }, { 0.9f, 0.2f, 0.3f }, { 0.4f, 0.8f, 0.7f } }, vcolors, vemissions;
	mvrt::PathTracer pt;
	pt.setup( stream );
	pt.setAOVs( true ); // before the frame exists: allocated by the resize
	pt.resizeFrameBufferIfNeeded( stream, 64, 36 );
	std::printf( "views %d %d bytes %lld %lld\n", (int)( pt.m_aovAlbedoF32 != nullptr ), (int)( pt.m_aovNormalDepthF32 != nullptr ), (long long)pt.m_aovAlbedoF32->bytes(),
				 (long long)pt.m_aovNormalDepthF32->bytes() );
	pt.loadHDRI( stream, "monks_forest_s.hdr" );
	pt.updateScene( vertices, vcolors, vemissions, stream, V3{ 0, 0, 0 }, 1.0f / 64, 64 );
	const float view[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.5f, -0.5f, -3, 1 };
	const float proj[16] = { 1.3f, 0, 0, 0, 0, 2.4f, 0, 0, 0, 0, -1, -1, 0, 0, -0.2f, 0 };
	pt.clearFrameBuffer( stream );
	pt.step( stream, view, proj, 3.0f, 0.01f );
	// a caller's own read of the device views: join first, like for m_frameBufferF32
	mvrt::check( mvrt_pt_join( pt.handle(), stream ), "join" );
	std::vector<float> albedo( 64 * 36 * 4 ), nd( 64 * 36 * 4 ), viaRead( 64 * 36 * 4 );
	mvrt::check( mvrt_memcpy_d2h( albedo.data(), pt.m_aovAlbedoF32->data(), albedo.size() * 4, stream ), "d2h" );
	mvrt::check( mvrt_memcpy_d2h( nd.data(), pt.m_aovNormalDepthF32->data(), nd.size() * 4, stream ), "d2h" );
	mvrt::check( mvrt_pt_read_aov( pt.handle(), stream, MVRT_AOV_ALBEDO, viaRead.data() ), "read_aov" );
	double hits = 0, t = 0;
	for( size_t i = 3; i < albedo.size(); i += 4 )
	{
		hits += albedo[i];
		t += nd[i];
	}
	std::printf( "hits %.0f positive t %d same %d\n", hits, (int)( t > 0 ), (int)( albedo == viaRead ) );
	pt.clearFrameBuffer( stream );
	pt.setAOVs( false );
	std::printf( "off %d %d dev %d\n", (int)( pt.m_aovAlbedoF32 == nullptr ), (int)( pt.m_aovNormalDepthF32 == nullptr ), (int)( mvrt_pt_aov_dev( pt.handle(), MVRT_AOV_ALBEDO ) == nullptr ) );
	pt.setAOVs( true );
	pt.setTile( 0, 2 ); // the library releases everything of the frame, the u8 buffer included: no stale view survives
	std::printf( "tile %d %d %d\n", (int)( pt.m_aovAlbedoF32 == nullptr ), (int)( pt.m_aovNormalDepthF32 == nullptr ), (int)( pt.m_frameBufferF32 == nullptr ) );
	pt.cleanUp();
	return 0;
}
