// lane_walk_host.cpp -- the per-lane octree walk of include/mvrt/device.hpp (mvrt::DeviceOctree::walk) on the CPU: the header as it lies, behind the
// stand-in tests/cpp/hip_host/hip/hip_runtime.h, built by tests/test_lane_walk_cpu.py with g++ -ffp-contract=off (every product and sum rounded on its own, as the
// header's pragma asks of clang) and once more under -fsanitize=address,undefined.  Every array lives in a heap block of its exact size, the caller's stack holds
// view.levels entries and not one more: an index out of range is an error of the sanitized run.
//
//   lane_walk_host <input> <output>
//
// input:   u32 magic, u32 stackMode (0: the method's own stack, 1: the caller's), u32 hasLimits, u32 0, u64 nNodes, u64 nRays,
//          mvrt_device_octree (128 bytes; its pointers are set here), nNodes node lines of 64 bytes,
//          plain flavour only: masks[nNodes] u8, psumCold[nNodes * 8] u32,
//          ro[nRays * 3] f32, rd[nRays * 3] f32, isShadow[nRays] u8, hasLimits only: tMax[nRays] f32
// output:  t[nRays] f32, nMajor[nRays] i32, vIndex[nRays] u32, descents[nRays] u32 of intersectEx,
//          hasLimits only: the same four of intersectRangeEx, then occluded[nRays] u8 of occluded( ro, rd, tMax )
#include <mvrt/device.hpp>

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static const uint32_t kMagic = 0x4B4C574Cu; // "LWLK"

template <class T>
static std::vector<T> readArray( FILE* f, uint64_t n )
{
	std::vector<T> v( n );
	if( n && fread( v.data(), sizeof( T ), n, f ) != n )
	{
		fprintf( stderr, "lane_walk_host: the input ends early\n" );
		exit( 2 );
	}
	return v;
}
template <class T>
static void writeArray( FILE* f, const std::vector<T>& v )
{
	if( !v.empty() && fwrite( v.data(), sizeof( T ), v.size(), f ) != v.size() )
	{
		fprintf( stderr, "lane_walk_host: cannot write the output\n" );
		exit( 2 );
	}
}

int main( int argc, char** argv )
{
	if( argc != 3 )
	{
		fprintf( stderr, "usage: lane_walk_host <input> <output>\n" );
		return 2;
	}
	FILE* in = fopen( argv[1], "rb" );
	if( !in )
	{
		fprintf( stderr, "lane_walk_host: cannot open %s\n", argv[1] );
		return 2;
	}
	const std::vector<uint32_t> head = readArray<uint32_t>( in, 4 );
	const std::vector<uint64_t> counts = readArray<uint64_t>( in, 2 );
	const uint32_t stackMode = head[1];
	const bool hasLimits = head[2] != 0;
	const uint64_t nNodes = counts[0], n = counts[1];
	mvrt_device_octree view = readArray<mvrt_device_octree>( in, 1 )[0];
	const bool plain = view.flavour == MVRT_FLAVOUR_PLAIN;
	if( head[0] != kMagic || stackMode > 1 || view.structBytes != sizeof( mvrt_device_octree ) || ( !plain && view.flavour != MVRT_FLAVOUR_EMBEDDED ) || view.levels < 1 ||
		view.levels > MVRT_DEVICE_MAX_LEVELS || nNodes == 0 || view.numberOfNodes != nNodes || view.rootIndex != nNodes - 1 )
	{
		fprintf( stderr, "lane_walk_host: not an input of this program\n" );
		return 2;
	}
	const std::vector<mvrt::detail::Line64> lines = readArray<mvrt::detail::Line64>( in, nNodes );
	const std::vector<uint8_t> masks = readArray<uint8_t>( in, plain ? nNodes : 0 );
	const std::vector<uint32_t> psumCold = readArray<uint32_t>( in, plain ? nNodes * 8 : 0 );
	const std::vector<float> ro = readArray<float>( in, n * 3 ), rd = readArray<float>( in, n * 3 );
	const std::vector<uint8_t> isShadow = readArray<uint8_t>( in, n );
	const std::vector<float> tMax = readArray<float>( in, hasLimits ? n : 0 );
	fclose( in );
	view.nodes = (uint64_t)(uintptr_t)lines.data();
	view.kids = 0;
	view.masks = plain ? (uint64_t)(uintptr_t)masks.data() : 0;
	view.psumCold = plain ? (uint64_t)(uintptr_t)psumCold.data() : 0;
	view.attrs = view.cellBlocks = view.cellEntries = 0;

	const mvrt::DeviceOctree oct( view );
	std::vector<mvrt::StackEntry> stack( view.levels );
	std::vector<float> t( n ), tR( hasLimits ? n : 0 );
	std::vector<int32_t> nMajor( n ), nMajorR( tR.size() );
	std::vector<uint32_t> vIndex( n ), descents( n ), vIndexR( tR.size() ), descentsR( tR.size() );
	std::vector<uint8_t> occluded( tR.size() );
	for( uint64_t i = 0; i < n; i++ )
	{
		const float3 o = make_float3( ro[3 * i], ro[3 * i + 1], ro[3 * i + 2] ), d = make_float3( rd[3 * i], rd[3 * i + 1], rd[3 * i + 2] );
		const bool sh = isShadow[i] != 0;
		int nm;
		if( stackMode == 1 ) oct.intersectEx( stack.data(), o, d, &t[i], &nm, &vIndex[i], sh, &descents[i] );
		else oct.intersectEx( o, d, &t[i], &nm, &vIndex[i], sh, &descents[i] );
		nMajor[i] = nm;
		if( !hasLimits ) continue;
		if( stackMode == 1 )
		{
			oct.intersectRangeEx( stack.data(), o, d, tMax[i], &tR[i], &nm, &vIndexR[i], sh, &descentsR[i] );
			occluded[i] = oct.occluded( stack.data(), o, d, tMax[i] ) ? 1 : 0;
		}
		else
		{
			oct.intersectRangeEx( o, d, tMax[i], &tR[i], &nm, &vIndexR[i], sh, &descentsR[i] );
			occluded[i] = oct.occluded( o, d, tMax[i] ) ? 1 : 0;
		}
		nMajorR[i] = nm;
	}

	FILE* out = fopen( argv[2], "wb" );
	if( !out )
	{
		fprintf( stderr, "lane_walk_host: cannot open %s\n", argv[2] );
		return 2;
	}
	writeArray( out, t );
	writeArray( out, nMajor );
	writeArray( out, vIndex );
	writeArray( out, descents );
	writeArray( out, tR );
	writeArray( out, nMajorR );
	writeArray( out, vIndexR );
	writeArray( out, descentsR );
	writeArray( out, occluded );
	return fclose( out ) == 0 ? 0 : 2;
}
