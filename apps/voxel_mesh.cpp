// voxel_mesh -- the reference voxelizer's "Save As Mesh" (voxMesh.cpp:111-219) without the GUI: voxelize a Wavefront .obj on the GPU and write the exposed
// faces of the voxel set as a PLY quad mesh, one colour per face from its voxel.
//
//   voxel_mesh scene.obj gridRes out.ply [--no-weld] [--merge | --merge-any] [--conservative]
//
// Default: shared vertices (mvrt_svo_surface_mesh).  --no-weld: four vertices of its own per face, like the reference's file (mvrt_svo_surface_quads);
// the positions are the same bit patterns either way.  --merge: coplanar faces of equal attribute become rectangles (mvrt_svo_surface_merged); --merge-any:
// whatever their attributes, each rectangle in the colour of its anchor voxel.  Both combine with --no-weld; a welded merged mesh has T-junctions (mvrt.h).
// Grid placement: bounding box of the mesh, dps = longest side / gridRes (voxPTGPU.cpp:159-163).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"
#include "scene_io.hpp"

int main( int argc, char** argv )
{
	bool weld = true, conservative = false, merge = false, mergeAny = false;
	std::vector<const char*> pos;
	for( int i = 1; i < argc; i++ )
	{
		if( !std::strcmp( argv[i], "--no-weld" ) ) weld = false;
		else if( !std::strcmp( argv[i], "--merge" ) ) merge = true;
		else if( !std::strcmp( argv[i], "--merge-any" ) ) merge = mergeAny = true;
		else if( !std::strcmp( argv[i], "--conservative" ) ) conservative = true;
		else pos.push_back( argv[i] );
	}
	if( pos.size() != 3 )
	{
		std::printf( "usage: voxel_mesh scene.obj gridRes out.ply [--no-weld] [--merge | --merge-any] [--conservative]\n"
					 "  --no-weld    four vertices of its own per face instead of shared ones\n"
					 "  --merge      merge coplanar faces of equal colour and emission into rectangles\n"
					 "  --merge-any  merge whatever the attributes; a rectangle takes the colour of its anchor voxel\n" );
		return pos.empty() ? 0 : 2;
	}
	const int gridRes = std::atoi( pos[1] );
	std::vector<mvrt_io::V3> vertices, vcolors, vemissions;
	if( !mvrt_io::readObj( pos[0], &vertices, &vcolors, &vemissions ) )
	{
		std::fprintf( stderr, "voxel_mesh: cannot read triangles from %s\n", pos[0] );
		return 1;
	}
	mvrt_io::V3 origin;
	float dps;
	mvrt_io::boundingGrid( vertices, gridRes, &origin, &dps );

	void* stream = nullptr;
	mvrt::IntersectorOctreeGPU svo;
	svo.build( vertices, vcolors, vemissions, nullptr, stream, origin, dps, gridRes, conservative ? MVRT_BUILD_CONSERVATIVE : 0 );
	std::vector<uint32_t> xyz, attribs;
	svo.readVoxels( xyz, attribs, stream );

	std::vector<float> points;
	std::vector<uint32_t> indices, faceVoxel;
	std::vector<uint8_t> faceDir;
	uint64_t nFaces = 0;
	if( merge )
	{
		std::vector<uint32_t> rectSize;
		nFaces = svo.surfaceMerged( ( mergeAny ? MVRT_SURFACE_MERGE_ANY_ATTRIBUTE : 0u ) | ( weld ? MVRT_SURFACE_MERGE_WELD : 0u ), points, indices, faceVoxel, faceDir, rectSize, stream );
	}
	else if( weld )
		svo.surfaceMesh( points, indices, faceVoxel, faceDir, stream );
	else
		svo.surfaceQuads( faceVoxel, faceDir, points, stream );
	if( !weld ) // four corners of its own per face or rectangle
	{
		if( faceVoxel.size() * 4ull > 0xFFFFFFFFull )
		{
			std::fprintf( stderr, "voxel_mesh: %zu faces have more corners than a PLY uint index can name\n", faceVoxel.size() );
			return 1;
		}
		indices.resize( faceVoxel.size() * 4 );
		for( size_t i = 0; i < indices.size(); i++ ) indices[i] = (uint32_t)i;
	}
	if( !mvrt_io::writePlyQuads( pos[2], points.data(), points.size() / 3, indices.data(), faceVoxel.data(), faceVoxel.size(),
								 reinterpret_cast<const uint8_t*>( attribs.data() ) ) )
	{
		std::fprintf( stderr, "voxel_mesh: cannot write %s\n", pos[2] );
		return 1;
	}
	if( merge )
		std::printf( "voxels %u faces %llu rects %zu vertices %zu -> %s\n", svo.m_numberOfVoxels, (unsigned long long)nFaces, faceVoxel.size(), points.size() / 3, pos[2] );
	else
		std::printf( "voxels %u faces %zu vertices %zu -> %s\n", svo.m_numberOfVoxels, faceVoxel.size(), points.size() / 3, pos[2] );
	return 0;
}
