// rtcamp_batch.cpp -- batch animation renderer on top of the drop-in boundary, following the structure of the
// reference's RTCamp.cpp: `--frame-range a b` sharding across machines (RTCamp.cpp:47-52 and
// usecase2_submission/run.py), per-frame SVO rebuild with a voxel-resolution ramp rounded up to a power of two
// (:136-142), clearFrameBuffer + N x step + resolve per frame (:153-166), and a worker thread that reads frames back
// through a 4-buffer pool and writes image files while the GPU renders the next frame (:126-130,165-193).
//
// The Alembic scene / camera animation of the reference (prlib, absent) is replaced by a Wavefront .obj mesh and an
// orbiting look-at camera.  Everything GPU-side goes through include/mvrt/PathTracer.hpp -> libmvrt_hip.so.
//
//   rtcamp_batch scene.obj env.hdr outdir [--frame-range a b] [--frames N] [--size W H] [--res from to] [--steps K] [--png] [--aov] [--denoise]
//                [--adaptive threshold] [--adaptive-every K]
//
// --aov also writes, beside each frame, <frame>_albedo and <frame>_normal in the frame's format: the means over all samples of the first-hit
// feature buffers (mvrt.h "First-hit feature buffers"), what a denoiser takes as guides.  Encoded on the host from read-back data, in fp32:
// albedo byte = (int)( 255 * ( sum / samples ) + 0.5f ), normal byte = (int)( 255 * ( 0.5f * ( sum / samples ) + 0.5f ) + 0.5f ), alpha 255.
// --denoise switches the feature buffers and the luminance moments on and also writes <frame>_denoised in the frame's format: mvrt_pt_denoise with the
// default parameters on the accumulated frame, tone-mapped by mvrt_resolve_buffer like the frame itself (mvrt.h "Denoiser").
// --adaptive switches the luminance moments on and keeps sampling only where the frame has not converged (mvrt.h "Adaptive sampling"): the first
// minSamples / 16 = 2 steps sample every pixel; then, every K steps (--adaptive-every, default 2), mvrt_pt_error_mask with the threshold marks the pixels whose
// standard error still exceeds threshold * max( mean luminance, 0.01 ) and mvrt_pt_set_sample_mask restricts the steps to them.  A frame stops early when no
// pixel is marked.  Per frame it prints the steps taken and the samples spent against steps * pixels * 16.  Composes with --denoise (per-pixel sample counts).
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mvrt/PathTracer.hpp"
#include "scene_io.hpp"

static uint32_t next_power_of_two( uint32_t v ) // RTCamp.cpp:13-23
{
	v--;
	v |= v >> 1;
	v |= v >> 2;
	v |= v >> 4;
	v |= v >> 8;
	v |= v >> 16;
	v++;
	return v;
}

// look-at view matrix + GL perspective, column-major (what prlib's GetCameraMatrix hands to PathTracer::step)
static void lookAt( const float eye[3], const float at[3], float fovyDeg, float aspect, float view[16], float proj[16] )
{
	float f[3] = { at[0] - eye[0], at[1] - eye[1], at[2] - eye[2] };
	float fl = std::sqrt( f[0] * f[0] + f[1] * f[1] + f[2] * f[2] );
	for( float& c : f ) c /= fl;
	float up[3] = { 0, 1, 0 };
	float s[3] = { f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0] };
	float sl = std::sqrt( s[0] * s[0] + s[1] * s[1] + s[2] * s[2] );
	for( float& c : s ) c /= sl;
	float u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
	const float m[16] = { s[0], u[0], -f[0], 0, s[1], u[1], -f[1], 0, s[2], u[2], -f[2], 0,
						  -( s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2] ), -( u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2] ), f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2], 1 };
	std::memcpy( view, m, sizeof( m ) );
	const float t = 1.0f / std::tan( fovyDeg * 3.14159265f / 360.0f );
	const float p[16] = { t / aspect, 0, 0, 0, 0, t, 0, 0, 0, 0, -1.0002f, -1, 0, 0, -0.20002f, 0 };
	std::memcpy( proj, p, sizeof( p ) );
}

struct Job
{
	int frame;
	uint8_t* pixels;
	const char* suffix; // "" = the frame itself (pixels go back to the pool), else a feature image (pixels are freed)
};

// feature-buffer sums -> RGBA8; normal = false: v = sum / samples, true: v = 0.5f * ( sum / samples ) + 0.5f
static uint8_t* encodeAov( const std::vector<float>& sum, const std::vector<float>& frame, size_t nPixels, bool normal )
{
	uint8_t* out = new uint8_t[nPixels * 4];
	for( size_t p = 0; p < nPixels; p++ )
	{
		const float samples = frame[p * 4 + 3];
		for( int c = 0; c < 3; c++ )
		{
			float v = sum[p * 4 + c] / samples;
			if( normal ) v = 0.5f * v + 0.5f;
			const float b = 255.0f * v;
			out[p * 4 + c] = (uint8_t)(int)( b + 0.5f );
		}
		out[p * 4 + 3] = 255;
	}
	return out;
}

int main( int argc, char** argv )
{
	if( argc < 4 )
	{
		std::printf( "usage: rtcamp_batch scene.obj env.hdr outdir [--frame-range a b] [--frames N] [--size W H] [--res from to] [--steps K] [--png] [--aov] [--denoise]\n"
					 "                    [--adaptive threshold] [--adaptive-every K] [--lod K]\n"
					 "  --lod K    coarsen the tracer's octree in place by K levels after every scene build (mvrt_svo_coarsen): a preview at gridRes >> K\n"
					 "  --aov      also write <frame>_albedo and <frame>_normal (first-hit feature buffers)\n"
					 "  --denoise  also write <frame>_denoised (a-trous denoiser on the feature buffers and the luminance moments)\n"
					 "  --adaptive after 32 samples per pixel, sample only the pixels whose standard error exceeds threshold * mean luminance; re-marked every K steps (default 2)\n" );
		std::printf( "  [instance 0] rtcamp_batch ... --frame-range 0 171\n  [instance 1] rtcamp_batch ... --frame-range 171 240\n" );
		return 0;
	}
	const char* objPath = argv[1];
	const char* hdrPath = argv[2];
	const std::string outDir = argv[3];
	int totalFrames = 240, beginFrame = 0, endFrame = -1, W = 1440, H = 900, fromRes = 256, toRes = 8192, steps = 8; // RTCamp.cpp:42-45,136-137,156
	bool png = false, dumpCameras = false, aov = false, denoise = false;
	float adaptive = 0.0f; // > 0: the threshold of --adaptive
	int adaptiveEvery = 2;
	int lod = 0; // > 0: the levels of --lod
	const int adaptiveMinSamples = 32;
	for( int i = 4; i < argc; i++ )
	{
		if( !std::strcmp( argv[i], "--dump-cameras" ) ) dumpCameras = true;
		else if( !std::strcmp( argv[i], "--frame-range" ) && i + 2 < argc ) { beginFrame = std::atoi( argv[i + 1] ); endFrame = std::atoi( argv[i + 2] ); i += 2; }
		else if( !std::strcmp( argv[i], "--frames" ) && i + 1 < argc ) totalFrames = std::atoi( argv[++i] );
		else if( !std::strcmp( argv[i], "--size" ) && i + 2 < argc ) { W = std::atoi( argv[i + 1] ); H = std::atoi( argv[i + 2] ); i += 2; }
		else if( !std::strcmp( argv[i], "--res" ) && i + 2 < argc ) { fromRes = std::atoi( argv[i + 1] ); toRes = std::atoi( argv[i + 2] ); i += 2; }
		else if( !std::strcmp( argv[i], "--steps" ) && i + 1 < argc ) steps = std::atoi( argv[++i] );
		else if( !std::strcmp( argv[i], "--png" ) ) png = true;
		else if( !std::strcmp( argv[i], "--aov" ) ) aov = true;
		else if( !std::strcmp( argv[i], "--denoise" ) ) denoise = true;
		else if( !std::strcmp( argv[i], "--adaptive" ) && i + 1 < argc ) adaptive = (float)std::atof( argv[++i] );
		else if( !std::strcmp( argv[i], "--adaptive-every" ) && i + 1 < argc ) adaptiveEvery = std::atoi( argv[++i] );
		else if( !std::strcmp( argv[i], "--lod" ) && i + 1 < argc ) lod = std::atoi( argv[++i] );
	}
	if( endFrame < 0 ) endFrame = totalFrames;
	if( adaptiveEvery < 1 ) adaptiveEvery = 1;

	std::vector<mvrt_io::V3> vertices, vcolors, vemissions;
	if( !mvrt_io::readObj( objPath, &vertices, &vcolors, &vemissions ) )
	{
		std::fprintf( stderr, "cannot read %s\n", objPath );
		return 1;
	}
	// a light: the top 6 % of the mesh glows (so m_hasEmission exercises the extra-sample branch)
	mvrt_io::V3 lo, dummy;
	float dps0;
	mvrt_io::boundingGrid( vertices, 1, &lo, &dps0 );
	for( size_t i = 0; i < vertices.size(); i++ )
		if( vertices[i].y > lo.y + 0.94f * dps0 ) vemissions[i] = mvrt_io::V3{ 1.0f, 0.85f, 0.6f };
	(void)dummy;

	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "mvrt_stream_create" );
	char name[256];
	mvrt_device_name( name, sizeof( name ) );
	std::printf( "Device: %s\n", name );

	mvrt::PathTracer pt;
	pt.setup( stream );
	if( aov || denoise ) pt.setAOVs( true );
	if( denoise || adaptive > 0.0f ) pt.setMoments( true );
	pt.resizeFrameBufferIfNeeded( stream, W, H );
	uint8_t* maskDev = nullptr; // --adaptive: the error mask, one byte per owned pixel
	if( adaptive > 0.0f ) mvrt::check( mvrt_malloc( (void**)&maskDev, mvrt_pt_owned_pixels( pt.handle() ) ), "mvrt_malloc" );
	uint8_t* denoisedU8Dev = nullptr; // the tone-mapped denoised frame on the device
	if( denoise ) mvrt::check( mvrt_malloc( (void**)&denoisedU8Dev, (uint64_t)W * H * 4 ), "mvrt_malloc" );
	pt.loadHDRI( stream, hdrPath, hdrPath );

	// worker: image writer with a 4-buffer pool (RTCamp.cpp:126-130,174-193)
	std::mutex mu;
	std::condition_variable cv;
	std::deque<uint8_t*> pool;
	std::deque<Job> jobs;
	bool done = false;
	for( int i = 0; i < 4; i++ ) pool.push_back( new uint8_t[(size_t)W * H * 4] );
	std::thread writer( [&]() {
		for( ;; )
		{
			Job j;
			{
				std::unique_lock<std::mutex> lk( mu );
				cv.wait( lk, [&] { return done || !jobs.empty(); } );
				if( jobs.empty() ) return;
				j = jobs.front();
				jobs.pop_front();
			}
			char file[512];
			std::snprintf( file, sizeof( file ), "%s/%03d%s.%s", outDir.c_str(), j.frame, j.suffix, png ? "png" : "ppm" );
			if( png ) mvrt_io::writePngUncompressed( file, j.pixels, W, H );
			else mvrt_io::writePpm( file, j.pixels, W, H );
			if( j.suffix[0] )
			{
				delete[] j.pixels;
				continue;
			}
			{
				std::lock_guard<std::mutex> lk( mu );
				pool.push_back( j.pixels );
			}
			cv.notify_all();
		}
	} );

	const float boxWide = dps0; // largest extent of the mesh
	const float centre[3] = { lo.x + 0.5f * boxWide, lo.y + 0.5f * boxWide, lo.z + 0.5f * boxWide };
	for( int frame = beginFrame; frame < endFrame; frame++ )
	{
		// voxel size ramps linearly from boxWide/fromRes to boxWide/toRes over the whole animation (RTCamp.cpp:138-142)
		const float tt = (float)frame / (float)totalFrames;
		const float dps = ( boxWide / fromRes ) + ( ( boxWide / toRes ) - ( boxWide / fromRes ) ) * tt;
		const int resolution = (int)std::ceil( boxWide / dps );
		const int gridRes = (int)next_power_of_two( (uint32_t)resolution );
		pt.updateScene( vertices, vcolors, vemissions, stream, lo, dps, gridRes );
		if( lod > 0 )
		{
			const uint32_t fine = pt.m_intersectorOctreeGPU.m_numberOfVoxels;
			pt.m_intersectorOctreeGPU.coarsen( lod, 1, 0, nullptr, stream );
			std::printf( "lod: voxels %u -> %u, gridRes %d -> %d\n", fine, pt.m_intersectorOctreeGPU.m_numberOfVoxels, gridRes, gridRes >> lod );
		}

		const float ang = 6.2831853f * tt;
		const float eye[3] = { centre[0] + 1.6f * boxWide * std::cos( ang ), centre[1] + 0.5f * boxWide, centre[2] + 1.6f * boxWide * std::sin( ang ) };
		float view[16], proj[16];
		lookAt( eye, centre, 40.0f, (float)W / (float)H, view, proj );
		const float focus = 1.6f * boxWide, lensR = 0.004f * boxWide;
		if( dumpCameras ) // exact inputs of this frame (hex floats) so that a test can replay it through another binding
		{
			char file[512];
			std::snprintf( file, sizeof( file ), "%s/%03d.camera.txt", outDir.c_str(), frame );
			if( FILE* fp = std::fopen( file, "w" ) )
			{
				for( int k = 0; k < 16; k++ ) std::fprintf( fp, "%a ", view[k] );
				std::fprintf( fp, "\n" );
				for( int k = 0; k < 16; k++ ) std::fprintf( fp, "%a ", proj[k] );
				std::fprintf( fp, "\n%a %a %a %a %a %a %d\n", focus, lensR, lo.x, lo.y, lo.z, dps, gridRes );
				std::fclose( fp );
			}
		}

		pt.clearFrameBuffer( stream );
		int taken = 0;
		uint64_t spent = 0; // samples
		for( int iteration = 0; iteration < steps; iteration++ )
		{
			const int sinceFull = iteration - adaptiveMinSamples / 16; // the first minSamples / 16 steps sample every pixel
			if( adaptive > 0.0f && sinceFull >= 0 && sinceFull % adaptiveEvery == 0 )
			{
				pt.errorMask( stream, adaptive, maskDev, 0.01f, adaptiveMinSamples );
				if( pt.setSampleMask( stream, maskDev ) == 0 ) break; // converged everywhere
			}
			pt.step( stream, view, proj, focus, lensR );
			taken++;
			spent += pt.activePixels() * 16;
		}

		uint8_t* buf = nullptr;
		{
			std::unique_lock<std::mutex> lk( mu );
			cv.wait( lk, [&] { return !pool.empty(); } );
			buf = pool.front();
			pool.pop_front();
		}
		pt.toImageAsync( stream, buf ); // resolve + DtoH (PathTracer.hpp:118-129)
		mvrt::check( mvrt_stream_synchronize( stream ), "sync" );
		uint8_t *albedoImage = nullptr, *normalImage = nullptr;
		if( aov ) // an optional output, not a hot path: read the sums back and encode them here, the writer thread does the files
		{
			const size_t owned = (size_t)mvrt_pt_owned_pixels( pt.handle() );
			std::vector<float> fb( owned * 4 ), sum( owned * 4 );
			mvrt::check( mvrt_pt_read_framebuffer( pt.handle(), stream, fb.data() ), "read_framebuffer" );
			mvrt::check( mvrt_pt_read_aov( pt.handle(), stream, MVRT_AOV_ALBEDO, sum.data() ), "read_aov" );
			albedoImage = encodeAov( sum, fb, (size_t)W * H, false );
			mvrt::check( mvrt_pt_read_aov( pt.handle(), stream, MVRT_AOV_NORMAL_DEPTH, sum.data() ), "read_aov" );
			normalImage = encodeAov( sum, fb, (size_t)W * H, true );
		}
		uint8_t* denoisedImage = nullptr;
		if( denoise )
		{
			pt.denoise( stream );
			mvrt::check( mvrt_resolve_buffer( (const float*)pt.m_denoisedF32->data(), (uint64_t)W * H, denoisedU8Dev, stream ), "mvrt_resolve_buffer" );
			denoisedImage = new uint8_t[(size_t)W * H * 4];
			mvrt::check( mvrt_memcpy_d2h( denoisedImage, denoisedU8Dev, (uint64_t)W * H * 4, stream ), "mvrt_memcpy_d2h" );
			mvrt::check( mvrt_stream_synchronize( stream ), "sync" );
		}
		{
			std::lock_guard<std::mutex> lk( mu );
			jobs.push_back( Job{ frame, buf, "" } );
			if( denoise ) jobs.push_back( Job{ frame, denoisedImage, "_denoised" } );
			if( aov )
			{
				jobs.push_back( Job{ frame, albedoImage, "_albedo" } );
				jobs.push_back( Job{ frame, normalImage, "_normal" } );
			}
		}
		cv.notify_all();
		std::printf( "[frame %d] res( %d -> grid %d ) voxels %llu octree %.1f MB\n", frame, resolution, gridRes, (unsigned long long)pt.getNumberOfVoxels(), pt.getOctreeBytes() / 1e6 );
		if( adaptive > 0.0f )
			std::printf( "[frame %d] adaptive: %d of %d steps, %llu of %llu samples\n", frame, taken, steps, (unsigned long long)spent, (unsigned long long)steps * (uint64_t)W * H * 16 );
	}
	{
		std::lock_guard<std::mutex> lk( mu );
		done = true;
	}
	cv.notify_all();
	writer.join();
	for( uint8_t* p : pool ) delete[] p;
	pt.cleanUp();
	if( denoisedU8Dev ) mvrt_free( denoisedU8Dev );
	if( maskDev ) mvrt_free( maskDev );
	mvrt_stream_destroy( stream );
	std::printf( "done\n" );
	return 0;
}
