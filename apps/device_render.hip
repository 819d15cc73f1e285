// device_render.hip -- the reference's `render` kernel (voxKernel.cu:437-483) written as an application kernel on the public
// device API (include/mvrt/device.hpp) and nothing else: one primary ray through each pixel centre, normal colour or vertex colour,
// plus an optional shadow ray per hit towards a directional sun (a second intersect() in the same thread).
//
//   device_render scene.obj out.ppm [--size W H] [--res N] [--vertex-color] [--camera c0 ... c14] [--sun x y z] [--lod SCALE] [--dump prefix] [--bench N]
//
// The octree is built from the OBJ with mvrt_svo_build (grid = bounding cube of the mesh, apps/scene_io.hpp).  Without --camera the view
// frames the grid from (+0.6, +0.4, +0.6) grid extents off its centre.
// --sun x y z: for each hit, a shadow ray (isShadowRay = true) with origin o = ro + rd * t and direction (x, y, z), both computed per component
//   in fp32 without contraction (o.x = ro.x + rd.x * t); the pixel is halved if that ray hits anything.
// --lod SCALE: the image comes from a second application kernel, renderLod, on intersectCone and mvrt::DeviceLod: every pixel's ray stops at the octree level
//   whose cells are SCALE pixels wide where it enters them (coneA = 0, coneB = SCALE * 2 tanHthetaY / H, as mvrt_render_primary_lod), and a stopped ray takes
//   the mean colour of its cell from the attribute pyramid (mvrt_svo_lod_prepare).  It casts no shadow ray: --lod is refused together with --sun.
// --dump prefix: prefix.camera.txt (the 15 camera floats, %a), prefix.t.f32, prefix.nmajor.i32 (per pixel) and, with --sun, prefix.shadow.u8.
// --bench N: N interleaved rounds of this kernel and of mvrt_render_primary (the library's persistent traversal) on the same octree and
//   camera, timed with HIP events; prints one JSON line with the median and minimum ms per frame of each, and with --lod of renderLod as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <mvrt/device.hpp>

#include "scene_io.hpp"

#define RENDER_THREADS 256 // RENDER_NUMBER_OF_THREAD, renderCommon.hpp:13

__global__ void __launch_bounds__( RENDER_THREADS ) render( mvrt_device_octree view, mvrt::CameraPinhole pinhole, int W, int H, int showVertexColor, int useSun, float3 sun,
															 uchar4* frameBuffer, float* tOut, int* nMajorOut, uint8_t* shadowOut )
{
	MVRT_DEVICE_FP_STRICT
	const mvrt::DeviceOctree intersector( view );
	const uint32_t pixelIdx = blockIdx.x * RENDER_THREADS + threadIdx.x;
	if( pixelIdx >= (uint32_t)( W * H ) ) return;
	const int x = (int)( pixelIdx % W ), y = (int)( pixelIdx / W );
	float3 ro, rd;
	pinhole.shoot( &ro, &rd, x, y, 0.5f, 0.5f, W, H );
	float t;
	int nMajor;
	uint32_t vIndex;
	intersector.intersect( ro, rd, &t, &nMajor, &vIndex, false );
	uchar4 colorOut = make_uchar4( 0, 0, 0, 255 );
	uint8_t shadowed = 0;
	if( t != MVRT_MAX_FLOAT )
	{
		if( showVertexColor )
			colorOut = intersector.getVoxelColor( vIndex );
		else
		{
			const float3 hitN = mvrt::getHitN( nMajor, rd );
			const float cx = ( hitN.x + 1.0f ) * 0.5f, cy = ( hitN.y + 1.0f ) * 0.5f, cz = ( hitN.z + 1.0f ) * 0.5f;
			colorOut = make_uchar4( (uint8_t)( 255 * cx + 0.5f ), (uint8_t)( 255 * cy + 0.5f ), (uint8_t)( 255 * cz + 0.5f ), 255 );
		}
		if( useSun )
		{
			const float3 o = make_float3( ro.x + rd.x * t, ro.y + rd.y * t, ro.z + rd.z * t );
			float ts;
			int nm;
			uint32_t vi;
			intersector.intersect( o, sun, &ts, &nm, &vi, true );
			shadowed = ts != MVRT_MAX_FLOAT ? 1 : 0;
			if( shadowed ) colorOut = make_uchar4( colorOut.x / 2, colorOut.y / 2, colorOut.z / 2, colorOut.w );
		}
	}
	frameBuffer[pixelIdx] = colorOut;
	if( tOut ) tOut[pixelIdx] = t;
	if( nMajorOut ) nMajorOut[pixelIdx] = nMajor;
	if( shadowOut ) shadowOut[pixelIdx] = shadowed;
}

// the same pixel through a cone: the walk stops at the pixel's own level of detail and the colour is the cell's, by its code
__global__ void __launch_bounds__( RENDER_THREADS ) renderLod( mvrt_device_octree view, mvrt_device_lod lodView, mvrt::CameraPinhole pinhole, int W, int H, int showVertexColor,
																float coneB, uchar4* frameBuffer, float* tOut, int* nMajorOut )
{
	MVRT_DEVICE_FP_STRICT
	const mvrt::DeviceOctree intersector( view );
	const mvrt::DeviceLod lod( lodView );
	const uint32_t pixelIdx = blockIdx.x * RENDER_THREADS + threadIdx.x;
	if( pixelIdx >= (uint32_t)( W * H ) ) return;
	const int x = (int)( pixelIdx % W ), y = (int)( pixelIdx / W );
	float3 ro, rd;
	pinhole.shoot( &ro, &rd, x, y, 0.5f, 0.5f, W, H );
	float t;
	int nMajor;
	uint32_t level, index;
	uint64_t cellCode;
	intersector.intersectCone( ro, rd, 0.0f, coneB, &t, &nMajor, &level, &cellCode );
	uchar4 colorOut = make_uchar4( 0, 0, 0, 255 );
	if( t != MVRT_MAX_FLOAT )
	{
		if( showVertexColor )
		{
			if( lod.lookup( level, cellCode, &index ) ) colorOut = lod.color( level, index );
		}
		else
		{
			const float3 hitN = mvrt::getHitN( nMajor, rd );
			const float cx = ( hitN.x + 1.0f ) * 0.5f, cy = ( hitN.y + 1.0f ) * 0.5f, cz = ( hitN.z + 1.0f ) * 0.5f;
			colorOut = make_uchar4( (uint8_t)( 255 * cx + 0.5f ), (uint8_t)( 255 * cy + 0.5f ), (uint8_t)( 255 * cz + 0.5f ), 255 );
		}
	}
	frameBuffer[pixelIdx] = colorOut;
	if( tOut ) tOut[pixelIdx] = t;
	if( nMajorOut ) nMajorOut[pixelIdx] = nMajor;
}

#define HIP_CHECK( e )                                                                           \
	do                                                                                           \
	{                                                                                            \
		hipError_t r_ = ( e );                                                                   \
		if( r_ != hipSuccess )                                                                   \
		{                                                                                        \
			std::fprintf( stderr, "%s failed: %s\n", #e, hipGetErrorString( r_ ) );             \
			return 1;                                                                            \
		}                                                                                        \
	} while( 0 )
#define MVRT_CHECK( e )                                                            \
	do                                                                             \
	{                                                                              \
		if( ( e ) != 0 )                                                           \
		{                                                                          \
			std::fprintf( stderr, "%s failed: %s\n", #e, mvrt_last_error() );      \
			return 1;                                                              \
		}                                                                          \
	} while( 0 )

template <class T>
static bool writeRaw( const std::string& path, const std::vector<T>& v )
{
	FILE* fp = std::fopen( path.c_str(), "wb" );
	if( !fp ) return false;
	const bool ok = std::fwrite( v.data(), sizeof( T ), v.size(), fp ) == v.size();
	std::fclose( fp );
	return ok;
}
static float median( std::vector<float> v )
{
	std::sort( v.begin(), v.end() );
	return v.empty() ? 0.0f : ( v.size() % 2 ? v[v.size() / 2] : 0.5f * ( v[v.size() / 2 - 1] + v[v.size() / 2] ) );
}

int main( int argc, char** argv )
{
	if( argc < 3 )
	{
		std::fprintf( stderr, "usage: %s scene.obj out.ppm [--size W H] [--res N] [--vertex-color] [--camera c0 ... c14] [--sun x y z] [--lod SCALE] [--dump prefix] [--bench N]\n", argv[0] );
		return 2;
	}
	int W = 1920, H = 1080, res = 256, vertexColor = 0, useSun = 0, bench = 0, haveCamera = 0, useLod = 0;
	float lodScale = 0.0f;
	float cam[15] = {};
	float sun[3] = { 0, 0, 0 };
	std::string dump;
	for( int i = 3; i < argc; i++ )
	{
		const std::string a = argv[i];
		auto need = [&]( int k ) {
			if( i + k >= argc )
			{
				std::fprintf( stderr, "%s needs %d values\n", a.c_str(), k );
				std::exit( 2 );
			}
		};
		if( a == "--size" ) { need( 2 ); W = std::atoi( argv[++i] ); H = std::atoi( argv[++i] ); }
		else if( a == "--res" ) { need( 1 ); res = std::atoi( argv[++i] ); }
		else if( a == "--vertex-color" ) vertexColor = 1;
		else if( a == "--camera" ) { need( 15 ); for( int k = 0; k < 15; k++ ) cam[k] = std::strtof( argv[++i], nullptr ); haveCamera = 1; }
		else if( a == "--sun" ) { need( 3 ); for( int k = 0; k < 3; k++ ) sun[k] = std::strtof( argv[++i], nullptr ); useSun = 1; }
		else if( a == "--lod" ) { need( 1 ); lodScale = std::strtof( argv[++i], nullptr ); useLod = 1; }
		else if( a == "--dump" ) { need( 1 ); dump = argv[++i]; }
		else if( a == "--bench" ) { need( 1 ); bench = std::atoi( argv[++i] ); }
		else { std::fprintf( stderr, "unknown option %s\n", a.c_str() ); return 2; }
	}
	if( W <= 0 || H <= 0 || (long long)W * H > ( 1ll << 30 ) ) { std::fprintf( stderr, "bad --size\n" ); return 2; }
	if( useLod && useSun ) { std::fprintf( stderr, "--lod and --sun do not go together: the cone kernel casts no shadow ray\n" ); return 2; }

	std::vector<mvrt_io::V3> verts, cols, emis;
	if( !mvrt_io::readObj( argv[1], &verts, &cols, &emis ) ) { std::fprintf( stderr, "cannot read %s\n", argv[1] ); return 1; }
	mvrt_io::V3 origin;
	float dps;
	mvrt_io::boundingGrid( verts, res, &origin, &dps );
	const float o[3] = { origin.x, origin.y, origin.z };
	mvrt_svo* svo = nullptr;
	MVRT_CHECK( mvrt_svo_create( &svo ) );
	MVRT_CHECK( mvrt_svo_build( svo, &verts[0].x, &cols[0].x, &emis[0].x, verts.size(), nullptr, o, dps, res ) );
	mvrt_device_octree view;
	MVRT_CHECK( mvrt_svo_device_view( svo, &view ) );
	mvrt_device_lod lodView;
	std::memset( &lodView, 0, sizeof( lodView ) );
	if( useLod )
	{
		MVRT_CHECK( mvrt_svo_lod_prepare( svo, nullptr ) );
		MVRT_CHECK( mvrt_svo_lod_view( svo, &lodView ) );
	}

	if( !haveCamera ) // look at the grid's centre from (+0.6, +0.4, +0.6) extents away, fovy 45 degrees
	{
		const float ext = dps * (float)res;
		const float c[3] = { origin.x + 0.5f * ext, origin.y + 0.5f * ext, origin.z + 0.5f * ext };
		const float e[3] = { c[0] + 0.6f * ext * 1.6f, c[1] + 0.4f * ext * 1.6f, c[2] + 0.6f * ext * 1.6f };
		float f[3] = { c[0] - e[0], c[1] - e[1], c[2] - e[2] };
		const float fl = std::sqrt( f[0] * f[0] + f[1] * f[1] + f[2] * f[2] );
		for( float& v : f ) v /= fl;
		float r[3] = { -f[2], 0.0f, f[0] };
		const float rl = std::sqrt( r[0] * r[0] + r[2] * r[2] );
		r[0] /= rl;
		r[2] /= rl;
		const float u[3] = { r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0] };
		const float init[15] = { e[0], e[1], e[2], f[0], f[1], f[2], u[0], u[1], u[2], r[0], r[1], r[2], std::tan( 22.5f * 3.14159265f / 180.0f ), 0.0f, 1.0f };
		std::memcpy( cam, init, sizeof( cam ) );
	}
	const mvrt::CameraPinhole pinhole( cam );
	const float3 sunDir = make_float3( sun[0], sun[1], sun[2] );

	const size_t n = (size_t)W * H;
	uchar4* rgba = nullptr;
	float* tDev = nullptr;
	int* nmDev = nullptr;
	uint8_t* shDev = nullptr;
	HIP_CHECK( hipMalloc( &rgba, n * sizeof( uchar4 ) ) );
	HIP_CHECK( hipMalloc( &tDev, n * sizeof( float ) ) );
	HIP_CHECK( hipMalloc( &nmDev, n * sizeof( int ) ) );
	HIP_CHECK( hipMalloc( &shDev, n ) );
	const dim3 grid( (unsigned)( ( n + RENDER_THREADS - 1 ) / RENDER_THREADS ) );
	const float coneB = lodScale * ( ( 2.0f * cam[12] ) / (float)H );
	if( useLod ) hipLaunchKernelGGL( renderLod, grid, dim3( RENDER_THREADS ), 0, 0, view, lodView, pinhole, W, H, vertexColor, coneB, rgba, tDev, nmDev );
	else hipLaunchKernelGGL( render, grid, dim3( RENDER_THREADS ), 0, 0, view, pinhole, W, H, vertexColor, useSun, sunDir, rgba, tDev, nmDev, useSun ? shDev : nullptr );
	HIP_CHECK( hipGetLastError() );
	HIP_CHECK( hipDeviceSynchronize() );

	std::vector<uint8_t> host( n * 4 );
	HIP_CHECK( hipMemcpy( host.data(), rgba, n * 4, hipMemcpyDeviceToHost ) );
	if( !mvrt_io::writePpm( argv[2], host.data(), W, H ) ) { std::fprintf( stderr, "cannot write %s\n", argv[2] ); return 1; }
	if( !dump.empty() )
	{
		std::vector<float> t( n );
		std::vector<int> nm( n );
		HIP_CHECK( hipMemcpy( t.data(), tDev, n * 4, hipMemcpyDeviceToHost ) );
		HIP_CHECK( hipMemcpy( nm.data(), nmDev, n * 4, hipMemcpyDeviceToHost ) );
		FILE* fp = std::fopen( ( dump + ".camera.txt" ).c_str(), "w" );
		if( !fp ) return 1;
		for( int k = 0; k < 15; k++ ) std::fprintf( fp, "%a%c", cam[k], k == 14 ? '\n' : ' ' );
		std::fclose( fp );
		bool ok = writeRaw( dump + ".t.f32", t ) && writeRaw( dump + ".nmajor.i32", nm );
		if( useSun )
		{
			std::vector<uint8_t> sh( n );
			HIP_CHECK( hipMemcpy( sh.data(), shDev, n, hipMemcpyDeviceToHost ) );
			ok = ok && writeRaw( dump + ".shadow.u8", sh );
		}
		if( !ok ) { std::fprintf( stderr, "cannot write the dump files\n" ); return 1; }
	}

	if( bench > 0 )
	{
		uint8_t* rgbaLib = nullptr;
		HIP_CHECK( hipMalloc( &rgbaLib, n * 4 ) );
		hipEvent_t e0, e1, e2, e3;
		HIP_CHECK( hipEventCreate( &e0 ) );
		HIP_CHECK( hipEventCreate( &e1 ) );
		HIP_CHECK( hipEventCreate( &e2 ) );
		HIP_CHECK( hipEventCreate( &e3 ) );
		std::vector<float> own, lib, cone;
		for( int r = -2; r < bench; r++ ) // two warm-up rounds of each, then N timed rounds, interleaved
		{
			HIP_CHECK( hipEventRecord( e0, 0 ) );
			hipLaunchKernelGGL( render, grid, dim3( RENDER_THREADS ), 0, 0, view, pinhole, W, H, vertexColor, useSun, sunDir, rgba, (float*)nullptr, (int*)nullptr, (uint8_t*)nullptr );
			HIP_CHECK( hipEventRecord( e1, 0 ) );
			MVRT_CHECK( mvrt_render_primary( svo, cam, W, H, vertexColor, rgbaLib, nullptr, nullptr, nullptr, nullptr, nullptr ) );
			HIP_CHECK( hipEventRecord( e2, 0 ) );
			if( useLod )
			{
				hipLaunchKernelGGL( renderLod, grid, dim3( RENDER_THREADS ), 0, 0, view, lodView, pinhole, W, H, vertexColor, coneB, rgba, (float*)nullptr, (int*)nullptr );
				HIP_CHECK( hipEventRecord( e3, 0 ) );
			}
			HIP_CHECK( hipEventSynchronize( useLod ? e3 : e2 ) );
			float a = 0, b = 0, c = 0;
			HIP_CHECK( hipEventElapsedTime( &a, e0, e1 ) );
			HIP_CHECK( hipEventElapsedTime( &b, e1, e2 ) );
			if( useLod ) HIP_CHECK( hipEventElapsedTime( &c, e2, e3 ) );
			if( r >= 0 )
			{
				own.push_back( a );
				lib.push_back( b );
				if( useLod ) cone.push_back( c );
			}
		}
		char lodPart[160] = "";
		if( useLod )
			std::snprintf( lodPart, sizeof( lodPart ), ", \"lod_scale\": %g, \"lod_kernel_ms\": {\"median\": %.4f, \"min\": %.4f}", (double)lodScale, median( cone ),
						   *std::min_element( cone.begin(), cone.end() ) );
		std::printf( "{\"size\": [%d, %d], \"res\": %d, \"sun\": %s, \"rounds\": %d, \"device_kernel_ms\": {\"median\": %.4f, \"min\": %.4f}, "
					 "\"render_primary_ms\": {\"median\": %.4f, \"min\": %.4f}%s}\n",
					 W, H, res, useSun ? "true" : "false", bench, median( own ), *std::min_element( own.begin(), own.end() ), median( lib ), *std::min_element( lib.begin(), lib.end() ),
					 lodPart );
		HIP_CHECK( hipFree( rgbaLib ) );
	}
	HIP_CHECK( hipFree( rgba ) );
	HIP_CHECK( hipFree( tDev ) );
	HIP_CHECK( hipFree( nmDev ) );
	HIP_CHECK( hipFree( shDev ) );
	MVRT_CHECK( mvrt_svo_destroy( svo ) );
	return 0;
}
