// cone_walk_host.cpp -- the cone-limited walk of include/mvrt/device.hpp (mvrt::DeviceOctree::intersectCone / intersectConeEx) on the CPU: the header as it
// lies, behind the stand-in tests/cpp/hip_host/hip/hip_runtime.h, built by tests/test_cone_walk_cpu.py with g++ -ffp-contract=off and once more under
// -fsanitize=address,undefined, as tests/cpp/lane_walk_host.cpp is.  Every array lives in a heap block of its exact size and the caller's stack holds
// view.levels entries and not one more.
//
//   cone_walk_host <input> <output>
//
// input:   u32 magic, u32 stackMode (0: the method's own stack, 1: the caller's), u32 0, u32 0, u64 nNodes, u64 nRays,
//          mvrt_device_octree (128 bytes; its pointers are set here), nNodes node lines of 64 bytes,
//          plain flavour only: masks[nNodes] u8, psumCold[nNodes * 8] u32,
//          ro[nRays * 3] f32, rd[nRays * 3] f32, coneA[nRays] f32, coneB[nRays] f32
// output:  t[nRays] f32, nMajor[nRays] i32, level[nRays] u32, cellCode[nRays] u64, descents[nRays] u32 of intersectConeEx,
//          then the first four of intersectCone
#include <mvrt/device.hpp>

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static const uint32_t kMagic = 0x454E4F43u; // "CONE"

template <class T>
static std::vector<T> readArray( FILE* f, uint64_t n )
{
	std::vector<T> v( n );
	if( n && fread( v.data(), sizeof( T ), n, f ) != n )
	{
		fprintf( stderr, "cone_walk_host: the input ends early\n" );
		exit( 2 );
	}
	return v;
}
template <class T>
static void writeArray( FILE* f, const std::vector<T>& v )
{
	if( !v.empty() && fwrite( v.data(), sizeof( T ), v.size(), f ) != v.size() )
	{
		fprintf( stderr, "cone_walk_host: cannot write the output\n" );
		exit( 2 );
	}
}

int main( int argc, char** argv )
{
	if( argc != 3 )
	{
		fprintf( stderr, "usage: cone_walk_host <input> <output>\n" );
		return 2;
	}
	FILE* in = fopen( argv[1], "rb" );
	if( !in )
	{
		fprintf( stderr, "cone_walk_host: cannot open %s\n", argv[1] );
		return 2;
	}
	const std::vector<uint32_t> head = readArray<uint32_t>( in, 4 );
	const std::vector<uint64_t> counts = readArray<uint64_t>( in, 2 );
	const uint32_t stackMode = head[1];
	const uint64_t nNodes = counts[0], n = counts[1];
	mvrt_device_octree view = readArray<mvrt_device_octree>( in, 1 )[0];
	const bool plain = view.flavour == MVRT_FLAVOUR_PLAIN;
	if( head[0] != kMagic || stackMode > 1 || view.structBytes != sizeof( mvrt_device_octree ) || ( !plain && view.flavour != MVRT_FLAVOUR_EMBEDDED ) || view.levels < 1 ||
		view.levels > MVRT_DEVICE_MAX_LEVELS || nNodes == 0 || view.numberOfNodes != nNodes || view.rootIndex != nNodes - 1 )
	{
		fprintf( stderr, "cone_walk_host: not an input of this program\n" );
		return 2;
	}
	const std::vector<mvrt::detail::Line64> lines = readArray<mvrt::detail::Line64>( in, nNodes );
	const std::vector<uint8_t> masks = readArray<uint8_t>( in, plain ? nNodes : 0 );
	const std::vector<uint32_t> psumCold = readArray<uint32_t>( in, plain ? nNodes * 8 : 0 );
	const std::vector<float> ro = readArray<float>( in, n * 3 ), rd = readArray<float>( in, n * 3 );
	const std::vector<float> coneA = readArray<float>( in, n ), coneB = readArray<float>( in, n );
	fclose( in );
	view.nodes = (uint64_t)(uintptr_t)lines.data();
	view.kids = 0;
	view.masks = plain ? (uint64_t)(uintptr_t)masks.data() : 0;
	view.psumCold = plain ? (uint64_t)(uintptr_t)psumCold.data() : 0;
	view.attrs = view.cellBlocks = view.cellEntries = 0;

	const mvrt::DeviceOctree oct( view );
	std::vector<mvrt::StackEntry> stack( view.levels );
	std::vector<float> t( n ), t2( n );
	std::vector<int32_t> nMajor( n ), nMajor2( n );
	std::vector<uint32_t> level( n ), level2( n ), descents( n );
	std::vector<uint64_t> code( n ), code2( n );
	for( uint64_t i = 0; i < n; i++ )
	{
		const float3 o = make_float3( ro[3 * i], ro[3 * i + 1], ro[3 * i + 2] ), d = make_float3( rd[3 * i], rd[3 * i + 1], rd[3 * i + 2] );
		int nm, nm2;
		if( stackMode == 1 )
		{
			oct.intersectConeEx( stack.data(), o, d, coneA[i], coneB[i], &t[i], &nm, &level[i], &code[i], &descents[i] );
			oct.intersectCone( stack.data(), o, d, coneA[i], coneB[i], &t2[i], &nm2, &level2[i], &code2[i] );
		}
		else
		{
			oct.intersectConeEx( o, d, coneA[i], coneB[i], &t[i], &nm, &level[i], &code[i], &descents[i] );
			oct.intersectCone( o, d, coneA[i], coneB[i], &t2[i], &nm2, &level2[i], &code2[i] );
		}
		nMajor[i] = nm;
		nMajor2[i] = nm2;
	}

	FILE* out = fopen( argv[2], "wb" );
	if( !out )
	{
		fprintf( stderr, "cone_walk_host: cannot open %s\n", argv[2] );
		return 2;
	}
	writeArray( out, t );
	writeArray( out, nMajor );
	writeArray( out, level );
	writeArray( out, code );
	writeArray( out, descents );
	writeArray( out, t2 );
	writeArray( out, nMajor2 );
	writeArray( out, level2 );
	writeArray( out, code2 );
	return fclose( out ) == 0 ? 0 : 2;
}
