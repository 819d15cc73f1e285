// Compile-check of the resampling methods of the C++ mirror (include/mvrt/IntersectorOctreeGPU.hpp) and of the signatures of the three C calls; without an
// argument it checks the refusals that need no GPU.  With the argument `run` (on a GPU) an L-shaped set of 16^3 is listed under a quarter turn made by
// cellTransformFromWorld and resampled into a second handle at twice the resolution.  Built by tests/test_resample_mirror.py, which compares every printed line
// with the Python wrapper.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

static_assert( std::is_same<decltype( &mvrt_svo_resample_voxels ),
							int ( * )( const mvrt_svo*, const mvrt_cell_transform*, int, uint64_t, uint32_t*, uint32_t*, uint32_t*, uint64_t*, void* )>::value,
			   "mvrt_svo_resample_voxels" );
static_assert( std::is_same<decltype( &mvrt_svo_resample ),
							int ( * )( const mvrt_svo*, mvrt_svo*, const mvrt_cell_transform*, const float*, float, int, int, uint64_t*, void* )>::value,
			   "mvrt_svo_resample" );
static_assert( std::is_same<decltype( &mvrt_cell_transform_from_world ), int ( * )( const double*, const float*, float, const float*, float, mvrt_cell_transform* )>::value,
			   "mvrt_cell_transform_from_world" );
static_assert( MVRT_TRANSFORM_FRAC_BITS == 24 && sizeof( mvrt_cell_transform ) == 104 && offsetof( mvrt_cell_transform, m ) == 8 && offsetof( mvrt_cell_transform, t ) == 80,
			   "mvrt_cell_transform" );

static int expectRefusal( int rc, const char* words, const char* what )
{
	const char* e = mvrt_last_error();
	if( rc != 0 && e && std::strstr( e, words ) ) return 0;
	std::printf( "FAILED %s: rc %d, error \"%s\", wanted \"%s\"\n", what, rc, e ? e : "", words );
	return 1;
}

static unsigned long long checksum( const std::vector<uint32_t>& xyz, const std::vector<uint32_t>& attribs, const std::vector<uint32_t>& source )
{
	unsigned long long s = 0;
	for( size_t i = 0; i < source.size(); i++ )
		s += ( i + 1 ) * ( xyz[3 * i] + 17ull * xyz[3 * i + 1] + 289ull * xyz[3 * i + 2] + 4913ull * source[i] ) + attribs[2 * i] + 3ull * attribs[2 * i + 1];
	return s;
}

int main( int argc, char** argv )
{
	using Svo = mvrt::IntersectorOctreeGPU;
	const double turn[12] = { 0, -1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0 }; // a quarter turn about z, about the centre of the unit cube: (x, y) -> (1 - y, x)
	const mvrt_cell_transform xf = Svo::cellTransformFromWorld( turn, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16 );
	if( argc < 2 ) // the refusals the host makes before any GPU work
	{
		int bad = 0;
		mvrt_svo* h = nullptr;
		mvrt::check( mvrt_svo_create( &h ), "create" );
		uint64_t n = 0;
		const float origin[3] = { 0, 0, 0 };
		bad += expectRefusal( mvrt_svo_resample_voxels( nullptr, &xf, 16, 0, nullptr, nullptr, nullptr, &n, nullptr ), "null handle", "listing, null handle" );
		bad += expectRefusal( mvrt_svo_resample( nullptr, h, &xf, origin, 1.0f, 16, 0, &n, nullptr ), "null handle", "resample, null src" );
		bad += expectRefusal( mvrt_svo_resample( h, nullptr, &xf, origin, 1.0f, 16, 0, &n, nullptr ), "null handle", "resample, null dst" );
		bad += expectRefusal( mvrt_svo_resample_voxels( h, &xf, 16, 0, nullptr, nullptr, nullptr, &n, nullptr ), "no octree", "listing, empty handle" );
		bad += expectRefusal( mvrt_svo_resample( h, h, &xf, origin, 1.0f, 16, 0, &n, nullptr ), "no octree", "resample, empty handle" );
		bad += expectRefusal( mvrt_svo_resample( h, h, &xf, origin, 1.0f, 16, 4, &n, nullptr ), "unsupported flags", "resample, conservative flag" );
		mvrt_cell_transform out;
		const double singular[12] = { 1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0 };
		bad += expectRefusal( mvrt_cell_transform_from_world( singular, origin, 1.0f, origin, 1.0f, &out ), "singular", "from_world, singular" );
		bad += expectRefusal( mvrt_cell_transform_from_world( turn, origin, 0.0f, origin, 1.0f, &out ), "dps", "from_world, dps 0" );
		bad += xf.structBytes == sizeof( xf ) && xf.reserved == 0 && xf.m[1] == ( 1ll << 24 ) && xf.m[3] == -( 1ll << 24 ) && xf.m[8] == ( 1ll << 24 ) && xf.m[0] == 0 &&
					   xf.t[0] == 0 && xf.t[1] == 16 * ( 1ll << 25 ) && xf.t[2] == 0
				   ? 0
				   : 1; // the inverse of the turn: s = ( c_y, 16 - c_x ) in points
		mvrt_svo_destroy( h );
		std::printf( "usage: resample_usage run (%d host checks failed)\n", bad );
		return bad;
	}
	void* stream = nullptr;
	mvrt::check( mvrt_stream_create( &stream ), "stream" );
	Svo src, dst;
	std::vector<uint32_t> ell, colour;
	for( uint32_t z = 2; z < 5; z++ )
		for( uint32_t y = 1; y < 12; y++ )
			for( uint32_t x = 1; x < 14; x++ )
				if( y < 4 || x < 3 )
				{
					ell.insert( ell.end(), { x, y, z } );
					colour.insert( colour.end(), { 0x00000001u * x + 0x00000100u * y + 0x00010000u * z, x == 1 ? 0x00000700u : 0u } );
				}
	src.buildFromVoxels( ell, colour, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16, 0, stream );
	std::vector<uint32_t> xyz, attribs, source;
	src.resampleVoxels( xf, 16, xyz, attribs, source, stream );
	const uint64_t sized = src.resampleVoxels( xf, 16, 0, nullptr, nullptr, nullptr, stream );
	std::printf( "turn n %zu sized %llu of %u checksum %llu\n", source.size(), (unsigned long long)sized, src.m_numberOfVoxels, checksum( xyz, attribs, source ) );
	// the same turn onto a grid of twice the resolution in the same place: every voxel becomes a turned 2x2x2 block
	const mvrt_cell_transform fine = Svo::cellTransformFromWorld( turn, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, mvrt::vec3{ 0, 0, 0 }, 1.0f / 32 );
	const uint64_t n = src.resample( fine, mvrt::vec3{ 0, 0, 0 }, 1.0f / 32, 32, 0, &dst, stream );
	std::printf( "fine n %llu voxels %u emission %u dps %.9g source voxels %u\n", (unsigned long long)n, dst.m_numberOfVoxels, (unsigned)dst.hasEmission(), (double)dst.m_dps,
				 src.m_numberOfVoxels );
	const uint64_t self = src.resample( xf, mvrt::vec3{ 0, 0, 0 }, 1.0f / 16, 16 ); // in place
	std::printf( "self n %llu voxels %u\n", (unsigned long long)self, src.m_numberOfVoxels );
	mvrt::check( mvrt_stream_destroy( stream ), "stream" );
	return n == 8 * sized && self == sized ? 0 : 1;
}
