// Host-only driver of mvrt_io::writePlyQuads (apps/scene_io.hpp) for tests/test_surface_cpu.py:
//   ply_check in.bin out.ply
// in.bin: uint64 nVertices, nFaces, nVoxels (0 = no attributes: white faces); then vertices (3 floats each), indices (4 uint32 per face), faceVoxel (uint32 per
// face), attributes (8 bytes per voxel).
#include <cstdio>
#include <vector>

#include "scene_io.hpp"

int main( int argc, char** argv )
{
	if( argc != 3 ) return 2;
	FILE* fp = std::fopen( argv[1], "rb" );
	if( !fp ) return 1;
	uint64_t n[3];
	if( std::fread( n, 8, 3, fp ) != 3 ) return 1;
	std::vector<float> vertices( n[0] * 3 );
	std::vector<uint32_t> indices( n[1] * 4 ), faceVoxel( n[1] );
	std::vector<uint8_t> attribs( n[2] * 8 );
	bool ok = std::fread( vertices.data(), 12, n[0], fp ) == n[0] && std::fread( indices.data(), 16, n[1], fp ) == n[1] && std::fread( faceVoxel.data(), 4, n[1], fp ) == n[1] &&
			  std::fread( attribs.data(), 8, n[2], fp ) == n[2];
	std::fclose( fp );
	if( !ok ) return 1;
	return mvrt_io::writePlyQuads( argv[2], vertices.data(), n[0], indices.data(), faceVoxel.data(), n[1], n[2] ? attribs.data() : nullptr ) ? 0 : 1;
}
