// PathTracer.hpp -- header-only C++ mirror of the reference's PathTracer (reference PathTracer.hpp:14-170)
// over the C-ABI in include/mvrt.h.  Same method names and call order as the reference's callers use
// (voxPTGPU.cpp:88-193, RTCamp.cpp:111-169):
//
//     PathTracer pt;
//     pt.setup( stream, kernelPath, includeDir, isNvidia );      // last three ignored: no runtime compilation
//     pt.resizeFrameBufferIfNeeded( stream, w, h );
//     pt.loadHDRI( stream, "monks_forest_s.hdr", "monks_forest_2k_primary.hdr" );
//     pt.updateScene( vertices, vcolors, vemissions, stream, origin, dps, gridRes );
//     pt.step( stream, viewMatrix, projMatrix, focus, lensR );   // prlib's Camera3D -> the two matrices
//     pt.toImageAsync( stream, rgba8 );                          // pr::Image2DRGBA8 -> uint8_t*
//
// prlib types at the boundary are replaced by plain data: the camera is the (view, proj) pair that
// GetCameraMatrix produces in the reference (PathTracer.hpp:152-153), images are raw pointers.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "IntersectorOctreeGPU.hpp"

namespace mvrt
{
// What the reference's callers touch of hipUtil.hpp:48-74 `Buffer` on the frame buffers (RTCamp.cpp:169 `pt.m_frameBufferU8->data()`): a NON-owning view of
// a device buffer the library owns (it is re-pointed by resizeFrameBufferIfNeeded).
class Buffer
{
public:
	Buffer( void* ptr, int64_t bytes ) : m_bytes( bytes ), m_ptr( ptr ) {}
	int64_t bytes() const { return m_bytes; }
	char* data() { return (char*)m_ptr; }

private:
	int64_t m_bytes;
	void* m_ptr;
};

struct PathTracer
{
	PathTracer() {}
	~PathTracer() { cleanUp(); }
	PathTracer( const PathTracer& ) = delete;
	void operator=( const PathTracer& ) = delete;

	int getSteps() const { return m_handle ? mvrt_pt_get_steps( m_handle ) : 0; }					   // :33
	uint64_t getNumberOfVoxels() const { return m_handle ? mvrt_pt_get_number_of_voxels( m_handle ) : 0; } // :34-37
	uint64_t getOctreeBytes() const { return m_handle ? mvrt_pt_get_octree_bytes( m_handle ) : 0; }	   // :38-41

	// :43-69
	void setup( void* stream, const char* /*kernel*/ = nullptr, const char* /*includeDir*/ = nullptr, bool /*isNvidia*/ = false )
	{
		if( !m_handle )
		{
			check( mvrt_pt_create( &m_handle ), "mvrt_pt_create" );
			m_intersectorOctreeGPU.attach( mvrt_pt_intersector( m_handle ) );
		}
		check( mvrt_pt_setup( m_handle, stream ), "PathTracer::setup" );
	}
	void cleanUp() // :71-79
	{
		m_frameBufferU8.reset();
		m_frameBufferF32.reset();
		m_aovAlbedoF32.reset();
		m_aovNormalDepthF32.reset();
		m_momentsF32.reset();
		m_denoisedF32.reset();
		m_intersectorOctreeGPU.attach( nullptr );
		if( m_handle ) mvrt_pt_destroy( m_handle );
		m_handle = nullptr;
	}
	void resizeFrameBufferIfNeeded( void* stream, int width, int height ) // :81-97
	{
		check( mvrt_pt_resize_framebuffer_if_needed( m_handle, stream, width, height ), "PathTracer::resizeFrameBufferIfNeeded" );
		m_width = width;
		m_height = height;
		// :90-93 -- uchar4 / float4 per OWNED pixel (= every pixel unless setTile split the frame)
		const int64_t owned = (int64_t)mvrt_pt_owned_pixels( m_handle );
		m_frameBufferU8.reset( new Buffer( mvrt_pt_framebuffer_u8_dev( m_handle ), owned * 4 ) );
		m_frameBufferF32.reset( new Buffer( mvrt_pt_framebuffer_dev( m_handle ), owned * 16 ) );
		pointAOVs();
		pointMoments();
		pointDenoised(); // (a resize releases the denoised image)
		m_steps = mvrt_pt_get_steps( m_handle );
	}
	void clearFrameBuffer( void* stream ) // :98-102
	{
		check( mvrt_pt_clear_framebuffer( m_handle, stream ), "PathTracer::clearFrameBuffer" );
		m_steps = 0;
	}
	void loadHDRI( void* stream, const char* file, const char* filePrimary = 0 )													 // :104-116
	{
		check( mvrt_pt_load_hdri_file( m_handle, stream, file, filePrimary ), "PathTracer::loadHDRI" );
	}
	void toImageAsync( void* stream, uint8_t* rgba8 ) { check( mvrt_pt_to_image_async( m_handle, stream, rgba8 ), "PathTracer::toImageAsync" ); } // :118-129
	void resolve( void* stream ) { check( mvrt_pt_resolve( m_handle, stream ), "PathTracer::resolve" ); }										   // :130-137

	template <class V3>
	void updateScene( const std::vector<V3>& vertices, const std::vector<V3>& vcolors, const std::vector<V3>& vemissions, void* stream, V3 origin, float dps, int gridRes ) // :139-148
	{
		m_intersectorOctreeGPU.build( vertices, vcolors, vemissions, nullptr, stream, origin, dps, gridRes );
	}
	// :150-169; view/proj are the column-major 4x4 matrices GetCameraMatrix returns
	void step( void* stream, const float view[16], const float proj[16], float focus, float lensR )
	{
		check( mvrt_pt_step_matrices( m_handle, stream, view, proj, focus, lensR ), "PathTracer::step" );
		m_steps = mvrt_pt_get_steps( m_handle ); // :159 m_steps++
	}

	// multi-GPU extension (not in the reference): render only the 256-pixel blocks b with b % tileCount == tileIndex
	// (the library releases everything of the frame here, the u8 buffer included: no view survives, the next resizeFrameBufferIfNeeded points them again)
	void setTile( int tileIndex, int tileCount )
	{
		m_frameBufferU8.reset();
		m_frameBufferF32.reset();
		m_aovAlbedoF32.reset();
		m_aovNormalDepthF32.reset();
		m_momentsF32.reset();
		m_denoisedF32.reset();
		check( mvrt_pt_set_tile( m_handle, tileIndex, tileCount ), "PathTracer::setTile" );
	}

	// first-hit feature buffers (not in the reference; mvrt.h "First-hit feature buffers"): off by default, before or after resizeFrameBufferIfNeeded,
	// not while steps are accumulated (clearFrameBuffer first)
	void setAOVs( bool enable )
	{
		check( mvrt_pt_set_aovs( m_handle, enable ? 1 : 0 ), "PathTracer::setAOVs" );
		pointAOVs();
	}

	// luminance moments (not in the reference; mvrt.h "Luminance moments"): under the rules of setAOVs, independent of it
	void setMoments( bool enable )
	{
		const int rc = mvrt_pt_set_moments( m_handle, enable ? 1 : 0 );
		pointMoments(); // (a reallocation that fails leaves no frame: the views follow the library either way)
		pointAOVs();
		pointDenoised();
		if( !mvrt_pt_framebuffer_dev( m_handle ) ) m_frameBufferF32.reset();
		check( rc, "PathTracer::setMoments" );
	}
	// the a-trous denoiser (not in the reference; mvrt.h "Denoiser") on this handle's frame: needs setAOVs( true ), setMoments( true ), one tile and at least one
	// step.  params == nullptr: the defaults.  m_denoisedF32 views the result (float4 per pixel, xyz = mean radiance, w = 1); null when the call failed
	void denoise( void* stream, const mvrt_denoise_params* params = nullptr )
	{
		const int rc = mvrt_pt_denoise( m_handle, stream, params );
		pointDenoised();
		check( rc, "PathTracer::denoise" );
	}

	// adaptive sampling (not in the reference; mvrt.h "Adaptive sampling").  setSampleMask: one byte per owned pixel on the device, nonzero = the steps that follow
	// sample the pixel; nullptr = every pixel again.  Returns the number of active pixels.  clearFrameBuffer, a reallocating resize and setTile drop the mask
	uint64_t setSampleMask( void* stream, const uint8_t* maskDev )
	{
		uint64_t n = 0;
		check( mvrt_pt_set_sample_mask( m_handle, stream, maskDev, &n ), "PathTracer::setSampleMask" );
		return n;
	}
	uint64_t activePixels() const { return mvrt_pt_active_pixels( m_handle ); }
	// writes 1 to maskDev (one byte per owned pixel) where the standard error of the pixel's mean luminance exceeds threshold * max( mean, lumFloor ), or the pixel
	// has fewer than minSamples samples; 0 from maxSamples samples on (0 = no limit).  Needs setMoments( true ).  Returns the number of ones; sets no mask
	uint64_t errorMask( void* stream, float threshold, uint8_t* maskDev, float lumFloor = 0.01f, int minSamples = 32, int maxSamples = 0 )
	{
		uint64_t n = 0;
		check( mvrt_pt_error_mask( m_handle, stream, threshold, lumFloor, minSamples, maxSamples, maskDev, &n ), "PathTracer::errorMask" );
		return n;
	}

	mvrt_pt* handle() const { return m_handle; }

	IntersectorOctreeGPU m_intersectorOctreeGPU; // reference member m_intersectorOctreeGPU (:18), a value as there; bound to the handle's octree by setup()
	std::unique_ptr<Buffer> m_frameBufferU8;  // :23 (filled by resolve / toImageAsync); views, see Buffer above
	std::unique_ptr<Buffer> m_frameBufferF32; // :24
	std::unique_ptr<Buffer> m_aovAlbedoF32;		 // MVRT_AOV_ALBEDO, float4 per owned pixel; null while the feature buffers are off (setAOVs)
	std::unique_ptr<Buffer> m_aovNormalDepthF32; // MVRT_AOV_NORMAL_DEPTH
	std::unique_ptr<Buffer> m_momentsF32;		 // float4 per owned pixel { sum l, sum l * l, 0, 0 }; null while the moments are off (setMoments)
	// float4 per pixel of the frame; null before the first denoise(), after resizeFrameBufferIfNeeded reallocated, after setTile and after a denoise() that
	// failed -- it is re-pointed by every member that can make the library release or reallocate it, so it never names freed memory
	std::unique_ptr<Buffer> m_denoisedF32;
	int m_width = 0;
	int m_height = 0;
	int m_steps = 0; // :27

private:
	void pointAOVs()
	{
		m_aovAlbedoF32.reset();
		m_aovNormalDepthF32.reset();
		if( float* a = mvrt_pt_aov_dev( m_handle, MVRT_AOV_ALBEDO ) )
		{
			const int64_t owned = (int64_t)mvrt_pt_owned_pixels( m_handle );
			m_aovAlbedoF32.reset( new Buffer( a, owned * 16 ) );
			m_aovNormalDepthF32.reset( new Buffer( mvrt_pt_aov_dev( m_handle, MVRT_AOV_NORMAL_DEPTH ), owned * 16 ) );
		}
	}
	void pointMoments()
	{
		m_momentsF32.reset();
		if( float* m = mvrt_pt_moments_dev( m_handle ) ) m_momentsF32.reset( new Buffer( m, (int64_t)mvrt_pt_owned_pixels( m_handle ) * 16 ) );
	}
	void pointDenoised()
	{
		m_denoisedF32.reset();
		if( float* d = mvrt_pt_denoised_dev( m_handle ) ) m_denoisedF32.reset( new Buffer( d, (int64_t)m_width * m_height * 16 ) );
	}
	mvrt_pt* m_handle = nullptr;
};
} // namespace mvrt
