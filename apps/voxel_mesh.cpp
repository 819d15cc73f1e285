// voxel_mesh -- the reference voxelizer's "Save As Mesh" (voxMesh.cpp:111-219) without the GUI: voxelize a Wavefront .obj on the GPU and write the exposed
// faces of the voxel set as a PLY quad mesh, one colour per face from its voxel.
//
//   voxel_mesh scene.obj gridRes out.ply [--no-weld] [--merge | --merge-any] [--conservative] [--lod K [--lod-min-count C]] [--fill | --fill-nearest | --exterior]
//              [--solid]
//              [--dilate K | --erode K | --close K | --open K] [--element faces|cube] [--components] [--keep-largest K] [--min-component N]
//              [--round-dilate RHO | --round-erode RHO | --round-close RHO | --round-open RHO]
//              [--union | --intersect | --subtract | --xor other.obj [--rotate-b ax ay az deg] [--scale-b s] [--offset x y z] [--attrib-b]]
//              [--recolour-from other.obj [--recolour-max D] | --distance-to other.obj]
//              [--ao [samples] [--ao-radius voxels]] [--smooth K [--smooth-limit L] [--smooth-taubin]]
//
// Default: shared vertices (mvrt_svo_surface_mesh).  --no-weld: four vertices of its own per face, like the reference's file (mvrt_svo_surface_quads);
// the positions are the same bit patterns either way.  --merge: coplanar faces of equal attribute become rectangles (mvrt_svo_surface_merged); --merge-any:
// whatever their attributes, each rectangle in the colour of its anchor voxel.  Both combine with --no-weld; a welded merged mesh has T-junctions (mvrt.h).
// --ao: bake per-face ambient occlusion into the colours (mvrt_svo_surface_ao): of `samples` rays (a power of two up to 256, default 64; the number, if any,
// directly follows --ao) `open` leave the face unoccluded within --ao-radius voxels (default 8), and every colour byte c becomes (c * open + samples / 2) / samples.
// With and without --no-weld; not with --merge / --merge-any: the bake is per face and a rectangle has no single value.
// --fill: the empty cells enclosed by the voxel shell become white voxels before the surface is extracted (mvrt_svo_fill_enclosed), so the inner side of the
// shell, which no outside ray can see, is not written; a line reports the voxels before and after and the cell and region counts.  With every other flag.
// --exterior: the same faces as --fill writes, without touching the octree: the faces that look into an enclosed cell are dropped from the masks
// (mvrt_svo_surface_exterior_masks) and the mesh is extracted from those (mvrt_svo_surface_*_masked); a line reports the faces before and after.  With every
// other flag except --fill: one or the other.
// --fill-nearest: as --fill, but every filled cell takes the colour and emission of its nearest voxel (mvrt_svo_fill_enclosed_nearest): the lowest vIndex among
// the voxels at the exact smallest distance, whatever that distance.  At the place of --fill; the line also reports the deepest squared distance.  Not with
// --fill or --exterior.
// --solid: the same fill, applied to the scene's model straight after it is voxelised and BEFORE --union / --intersect / --subtract / --xor, so that the faces a
// second model cuts into it carry the colours of the shell: --solid --subtract other.obj.  With every other flag that --fill combines with.
// --lod K: the octree is coarsened in place by K levels (mvrt_svo_coarsen: gridRes >> K, a cell is a voxel when it holds at least --lod-min-count fine voxels,
// default 1) before anything else is done with it; a line reports voxels and gridRes before and after.  With every other flag.
// --dilate K, --erode K, --close K, --open K (one of them): K steps of the operator on the voxel set (mvrt_svo_dilate / _erode / _close / _open) with --element
// faces (the 6 face neighbours) or cube (the 26 of the 3x3x3 block, the default), after --lod and before --fill / --exterior; a line reports the voxels before
// and after.  --close 1 --fill repairs a shell with one-voxel holes, which the fill alone finds empty of enclosed cells.  With every other flag.
// --round-dilate RHO, --round-erode RHO, --round-close RHO, --round-open RHO (one of them, and none of the four above): the operator with the ball of squared
// radius RHO in [1, 1024] as one operation (mvrt_svo_dilate_ball / _erode_ball / _close_ball / _open_ball): a round offset, where K steps give an octahedron or
// a cube.  At the same place, after --lod and before --keep-largest / --fill / --exterior; a line reports the voxels before and after.  --round-close 16 --fill
// bridges gaps of up to 8 cells in every direction alike.  With every other flag.
// --components: a line reports the number of connected components under --element and the five largest sizes (mvrt_svo_components); nothing changes.
// --keep-largest K, --min-component N (either or both): only the components of at least N voxels and, of those, the K largest stay (mvrt_svo_keep_components
// with --element: cube = 26-connected, the default; faces = 6-connected); a line reports voxels and components before and after.  All three come after --dilate
// / --erode / --close / --open and before --fill / --exterior, --components first: it counts what the other two select from.  --close 1 --keep-largest 1 --fill
// repairs a shell, drops the debris around it and fills it.  With every other flag.
// --union other.obj, --intersect other.obj, --subtract other.obj, --xor other.obj (one of them): the voxel set of a second model is combined with that of the
// scene (mvrt_svo_combine) before --lod and everything behind it.  Both models are voxelised on one lattice, the grid placement below applied to their joint
// bounding box; --offset x y z moves the second set by whole cells first (what leaves the grid is clipped), --attrib-b gives the cells both models share the
// colour of the second.  A line reports the voxels before and after, the second model's voxels, the overlap and the clipped voxels.  With every other flag.
// --rotate-b ax ay az deg, --scale-b s (either or both, only with one of the four above): the second set is turned by deg degrees about the axis (ax, ay, az) and
// scaled by s > 0, both about the centre of the grid, before it is combined: resampled into a scratch octree on the same lattice (mvrt_svo_resample with the
// transform mvrt_cell_transform_from_world makes of the world matrix), no triangle is voxelised again.  A line reports the second set's voxels before and after;
// --offset still applies, to the resampled set.
// --recolour-from other.obj: the second model is voxelised on the joint grid exactly as for --union (--offset, --rotate-b and --scale-b apply as there) and
// every voxel of the scene takes the colour and emission of the nearest voxel of the second set (mvrt_svo_transfer_attributes): clean geometry coloured from a
// scan.  --recolour-max D limits the reach to D cells (maxDist2 = D * D); voxels further off keep their bytes.  A line reports the voxels changed and beyond.
// --distance-to other.obj: a line reports, for both directions, the largest distance from a voxel of the one set to the other set (the one-sided Hausdorff
// distance, mvrt_svo_nearest_between) as the root of the integer d2, the farthest voxel, the voxels at distance 0 and the voxel counts; the mesh is then written as
// without the flag.  Only one of these two and --union / --intersect / --subtract / --xor; they run at the place of the combine, before --lod and what follows.
// --smooth K: the welded mesh smoothed by K iterations of constrained surface nets (mvrt_svo_surface_smooth): the faces, indices and colours of the default
// mesh, every vertex relaxed towards the mean of its edge neighbours inside a box of --smooth-limit L / 256 cell (L in [0, 128], default 127: no two vertices
// can meet) around its lattice corner.  --smooth-taubin: the weights 128 / -136 of Taubin's non-shrinking pair instead of the plain 256 / 256.  The line of
// counts also reports the clamped count.  With every flag --exterior and --fill combine with (--exterior through the masks argument) and with --ao, whose bake
// stays per voxel face; not with --merge / --merge-any (merged rectangles have T-junctions) nor with --no-weld (unshared corners have no neighbours).
// Grid placement: bounding box of the mesh, dps = longest side / gridRes (voxPTGPU.cpp:159-163).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"
#include "scene_io.hpp"

int main( int argc, char** argv )
{
	bool weld = true, conservative = false, merge = false, mergeAny = false, ao = false, fill = false, exterior = false, fillNearest = false, solid = false;
	int aoSamples = 64;
	bool smooth = false, smoothTaubin = false, smoothLimitGiven = false;
	int smoothIterations = 0, smoothLimit = 127;
	float aoRadiusVoxels = 8.0f;
	int lod = 0;
	unsigned long long lodMinCount = 1;
	const char* morphOp = nullptr; // "dilate", "erode", "close" or "open"
	int morphSteps = 0, morphOps = 0, element = MVRT_MORPH_CUBE;
	const char* roundOp = nullptr; // "dilate", "erode", "close" or "open"
	long long roundRadius2 = 0;
	int roundOps = 0;
	bool elementOk = true, components = false;
	long long keepLargest = 0, minComponent = 1; // 0 = no --keep-largest
	bool keep = false, keepOk = true;
	const char *combineName = nullptr, *otherObj = nullptr; // "union", "intersect", "subtract" or "xor"
	int combineOps = 0, combineOp = 0, offset[3] = { 0, 0, 0 };
	bool recolour = false, distanceTo = false; // --recolour-from / --distance-to: at the place of the combine, with its second model
	long long recolourMax = -1;					// cells; -1 = no limit
	bool attribB = false, resampleB = false, resampleOk = true;
	double rotateB[4] = { 0.0, 0.0, 1.0, 0.0 }, scaleB = 1.0; // axis and degrees
	std::vector<const char*> pos;
	for( int i = 1; i < argc; i++ )
	{
		if( !std::strcmp( argv[i], "--no-weld" ) ) weld = false;
		else if( !std::strcmp( argv[i], "--merge" ) ) merge = true;
		else if( !std::strcmp( argv[i], "--merge-any" ) ) merge = mergeAny = true;
		else if( !std::strcmp( argv[i], "--conservative" ) ) conservative = true;
		else if( !std::strcmp( argv[i], "--fill" ) ) fill = true;
		else if( !std::strcmp( argv[i], "--exterior" ) ) exterior = true;
		else if( !std::strcmp( argv[i], "--fill-nearest" ) ) fillNearest = true;
		else if( !std::strcmp( argv[i], "--solid" ) ) solid = true;
		else if( !std::strcmp( argv[i], "--ao" ) )
		{
			ao = true;
			if( i + 1 < argc && argv[i + 1][0] && std::strspn( argv[i + 1], "0123456789" ) == std::strlen( argv[i + 1] ) ) aoSamples = std::atoi( argv[++i] );
		}
		else if( !std::strcmp( argv[i], "--ao-radius" ) && i + 1 < argc ) aoRadiusVoxels = (float)std::atof( argv[++i] );
		else if( !std::strcmp( argv[i], "--smooth" ) && i + 1 < argc )
		{
			smooth = true;
			smoothIterations = std::atoi( argv[++i] );
		}
		else if( !std::strcmp( argv[i], "--smooth-limit" ) && i + 1 < argc )
		{
			smoothLimitGiven = true;
			smoothLimit = std::atoi( argv[++i] );
		}
		else if( !std::strcmp( argv[i], "--smooth-taubin" ) ) smoothTaubin = true;
		else if( !std::strcmp( argv[i], "--lod" ) && i + 1 < argc ) lod = std::atoi( argv[++i] );
		else if( !std::strcmp( argv[i], "--lod-min-count" ) && i + 1 < argc ) lodMinCount = std::strtoull( argv[++i], nullptr, 10 );
		else if( ( !std::strcmp( argv[i], "--dilate" ) || !std::strcmp( argv[i], "--erode" ) || !std::strcmp( argv[i], "--close" ) || !std::strcmp( argv[i], "--open" ) ) && i + 1 < argc )
		{
			morphOp = argv[i] + 2;
			morphSteps = std::atoi( argv[++i] );
			morphOps++;
		}
		else if( ( !std::strcmp( argv[i], "--round-dilate" ) || !std::strcmp( argv[i], "--round-erode" ) || !std::strcmp( argv[i], "--round-close" ) ||
				   !std::strcmp( argv[i], "--round-open" ) ) &&
				 i + 1 < argc )
		{
			roundOp = argv[i] + 8;
			roundRadius2 = std::atoll( argv[++i] );
			roundOps++;
		}
		else if( ( !std::strcmp( argv[i], "--union" ) || !std::strcmp( argv[i], "--intersect" ) || !std::strcmp( argv[i], "--subtract" ) || !std::strcmp( argv[i], "--xor" ) ) &&
				 i + 1 < argc )
		{
			combineName = argv[i] + 2;
			combineOp = !std::strcmp( combineName, "union" )	   ? mvrt::IntersectorOctreeGPU::COMBINE_UNION
						: !std::strcmp( combineName, "intersect" ) ? mvrt::IntersectorOctreeGPU::COMBINE_INTERSECTION
						: !std::strcmp( combineName, "subtract" )  ? mvrt::IntersectorOctreeGPU::COMBINE_DIFFERENCE
																   : mvrt::IntersectorOctreeGPU::COMBINE_XOR;
			otherObj = argv[++i];
			combineOps++;
		}
		else if( ( !std::strcmp( argv[i], "--recolour-from" ) || !std::strcmp( argv[i], "--distance-to" ) ) && i + 1 < argc )
		{
			combineName = argv[i] + 2;
			( !std::strcmp( combineName, "recolour-from" ) ? recolour : distanceTo ) = true;
			otherObj = argv[++i];
			combineOps++;
		}
		else if( !std::strcmp( argv[i], "--recolour-max" ) && i + 1 < argc ) recolourMax = std::atoll( argv[++i] );
		else if( !std::strcmp( argv[i], "--offset" ) && i + 3 < argc )
		{
			for( int k = 0; k < 3; k++ ) offset[k] = std::atoi( argv[++i] );
		}
		else if( !std::strcmp( argv[i], "--attrib-b" ) ) attribB = true;
		else if( !std::strcmp( argv[i], "--rotate-b" ) && i + 4 < argc )
		{
			for( int k = 0; k < 4; k++ ) rotateB[k] = std::atof( argv[++i] );
			resampleB = true;
			resampleOk = resampleOk && rotateB[0] * rotateB[0] + rotateB[1] * rotateB[1] + rotateB[2] * rotateB[2] > 0.0;
		}
		else if( !std::strcmp( argv[i], "--scale-b" ) && i + 1 < argc )
		{
			scaleB = std::atof( argv[++i] );
			resampleB = true;
			resampleOk = resampleOk && scaleB > 0.0 && scaleB - scaleB == 0.0;
		}
		else if( !std::strcmp( argv[i], "--components" ) ) components = true;
		else if( !std::strcmp( argv[i], "--keep-largest" ) && i + 1 < argc )
		{
			keepLargest = std::atoll( argv[++i] );
			keep = true;
			keepOk = keepOk && keepLargest >= 1 && keepLargest <= 0xFFFFFFFFll;
		}
		else if( !std::strcmp( argv[i], "--min-component" ) && i + 1 < argc )
		{
			minComponent = std::atoll( argv[++i] );
			keep = true;
			keepOk = keepOk && minComponent >= 1;
		}
		else if( !std::strcmp( argv[i], "--element" ) && i + 1 < argc )
		{
			i++;
			if( !std::strcmp( argv[i], "faces" ) ) element = MVRT_MORPH_FACES;
			else if( !std::strcmp( argv[i], "cube" ) ) element = MVRT_MORPH_CUBE;
			else elementOk = false;
		}
		else pos.push_back( argv[i] );
	}
	if( pos.size() != 3 )
	{
		std::printf( "usage: voxel_mesh scene.obj gridRes out.ply [--no-weld] [--merge | --merge-any] [--conservative] [--lod K [--lod-min-count C]]\n"
					 "                  [--fill | --fill-nearest | --exterior] [--solid]\n"
					 "                  [--dilate K | --erode K | --close K | --open K] [--element faces|cube] [--components] [--keep-largest K] [--min-component N]\n"
					 "                  [--round-dilate RHO | --round-erode RHO | --round-close RHO | --round-open RHO]\n"
					 "                  [--union | --intersect | --subtract | --xor other.obj [--rotate-b ax ay az deg] [--scale-b s] [--offset x y z] [--attrib-b]]\n"
					 "                  [--recolour-from other.obj [--recolour-max D] | --distance-to other.obj]\n"
					 "                  [--ao [samples] [--ao-radius voxels]] [--smooth K [--smooth-limit L] [--smooth-taubin]]\n"
					 "  --union O, --intersect O, --subtract O, --xor O  combine the voxel set with that of a second model O.obj first, both voxelised on one grid\n"
					 "               over their joint bounding box; --offset x y z moves the second set by whole cells, --attrib-b colours shared cells from it\n"
					 "  --rotate-b ax ay az deg, --scale-b s  turn the second voxel set by deg degrees about the axis and scale it by s > 0, about the grid centre,\n"
					 "               before it is combined (resampled on the GPU; only with one of the four options above)\n"
					 "  --recolour-from O  every voxel takes colour and emission of the nearest voxel of a second model O.obj, voxelised as for --union (--offset,\n"
					 "               --rotate-b, --scale-b apply); --recolour-max D: only within D cells.  --distance-to O  report the largest distance between the two\n"
					 "               voxel sets in both directions; the mesh is written as without it.  One of these and --union / --intersect / --subtract / --xor\n"
					 "  --lod K      coarsen the octree by K levels first (gridRes >> K); --lod-min-count C keeps a coarse cell only when it holds C fine voxels\n"
					 "  --dilate K   grow the voxel set by K layers; --erode K peels K layers; --close K = dilate K, erode K (plugs holes); --open K = erode K,\n"
					 "               dilate K (removes specks).  One of them, after --lod and before --fill / --exterior; --element faces|cube (default cube)\n"
					 "  --round-dilate RHO, --round-erode RHO, --round-close RHO, --round-open RHO  the same operators with the ball of squared radius RHO in\n"
					 "               [1, 1024] as one operation: a round offset.  One of them, at the same place, and none of the four above\n"
					 "  --components report the number of connected components (26-connected with --element cube, 6-connected with faces) and the five largest\n"
					 "  --keep-largest K, --min-component N  keep only the components of at least N voxels and, of those, the K largest; after the\n"
					 "               operators above and before --fill / --exterior\n"
					 "  --fill       fill the empty cells the voxel shell encloses (white voxels) before the surface is extracted\n"
					 "  --fill-nearest  the same fill, every cell in the colour of its nearest voxel, at the place of --fill.  Not with --fill or --exterior\n"
					 "  --solid      that fill on the scene's model straight after it is voxelised, before --union / --intersect / --subtract / --xor: the faces\n"
					 "               the second model cuts carry the colours of the shell\n"
					 "  --exterior   drop the faces that look into an enclosed cell instead; the octree stays as built.  Not with --fill\n"
					 "  --ao         bake ambient occlusion into the face colours: samples rays per face (power of two <= 256, default 64) within\n"
					 "               --ao-radius voxels (default 8); not with --merge / --merge-any\n"
					 "  --smooth K   smooth the welded mesh by K iterations (0..256) of constrained surface nets: same faces and indices, every vertex kept within\n"
					 "               --smooth-limit L / 256 cell (0..128, default 127) of its lattice corner; --smooth-taubin: the non-shrinking weights 128 / -136.\n"
					 "               With --exterior, --fill and --ao; not with --merge / --merge-any or --no-weld\n"
					 "  --no-weld    four vertices of its own per face instead of shared ones\n"
					 "  --merge      merge coplanar faces of equal colour and emission into rectangles\n"
					 "  --merge-any  merge whatever the attributes; a rectangle takes the colour of its anchor voxel\n" );
		return pos.empty() ? 0 : 2;
	}
	if( combineOps > 1 )
	{
		std::fprintf( stderr, "voxel_mesh: only one of --union / --intersect / --subtract / --xor / --recolour-from / --distance-to\n" );
		return 2;
	}
	if( recolourMax != -1 && ( !recolour || recolourMax < 0 || recolourMax > 8000000 ) )
	{
		std::fprintf( stderr, "voxel_mesh: --recolour-max D (D in [0, 8000000] cells) needs --recolour-from\n" );
		return 2;
	}
	if( resampleB && ( combineOps != 1 || !resampleOk ) )
	{
		std::fprintf( stderr, "voxel_mesh: --rotate-b ax ay az deg (an axis that is not zero) and --scale-b s (s > 0) need one of --union / --intersect / --subtract / --xor / --recolour-from / --distance-to\n" );
		return 2;
	}
	if( fill && exterior )
	{
		std::fprintf( stderr, "voxel_mesh: --exterior cannot be combined with --fill: one or the other (both write the same faces)\n" );
		return 2;
	}
	if( fillNearest && ( fill || exterior ) )
	{
		std::fprintf( stderr, "voxel_mesh: --fill-nearest cannot be combined with --fill or --exterior: one of the three\n" );
		return 2;
	}
	if( morphOps > 1 || !elementOk || ( morphOps == 1 && ( morphSteps < 1 || morphSteps > 64 ) ) )
	{
		std::fprintf( stderr, "voxel_mesh: one of --dilate / --erode / --close / --open with K in [1, 64], and --element faces or cube\n" );
		return 2;
	}
	if( roundOps > 1 || ( roundOps == 1 && ( morphOps != 0 || roundRadius2 < 1 || roundRadius2 > 1024 ) ) )
	{
		std::fprintf( stderr, "voxel_mesh: one of --round-dilate / --round-erode / --round-close / --round-open with RHO in [1, 1024], and not together with --dilate / "
							  "--erode / --close / --open\n" );
		return 2;
	}
	if( !keepOk )
	{
		std::fprintf( stderr, "voxel_mesh: --keep-largest needs K in [1, 2^32 - 1] and --min-component N >= 1\n" );
		return 2;
	}
	if( ao && merge )
	{
		std::fprintf( stderr, "voxel_mesh: --ao cannot be combined with --merge / --merge-any: the occlusion is baked per face and a rectangle has no single value\n" );
		return 2;
	}
	if( ao && ( aoSamples < 1 || aoSamples > 256 || ( aoSamples & ( aoSamples - 1 ) ) != 0 || !( aoRadiusVoxels > 0.0f ) ) )
	{
		std::fprintf( stderr, "voxel_mesh: --ao needs a power of two in [1, 256] and --ao-radius a value above 0\n" );
		return 2;
	}
	if( smooth && ( merge || !weld ) )
	{
		std::fprintf( stderr, "voxel_mesh: --smooth cannot be combined with --merge / --merge-any (merged rectangles have T-junctions) or with --no-weld (unshared corners "
							  "have no neighbours)\n" );
		return 2;
	}
	if( ( ( smoothTaubin || smoothLimitGiven ) && !smooth ) || ( smooth && ( smoothIterations < 0 || smoothIterations > 256 || smoothLimit < 0 || smoothLimit > 128 ) ) )
	{
		std::fprintf( stderr, "voxel_mesh: --smooth K with K in [0, 256]; --smooth-limit L (L in [0, 128]) and --smooth-taubin need it\n" );
		return 2;
	}
	const int gridRes = std::atoi( pos[1] );
	std::vector<mvrt_io::V3> vertices, vcolors, vemissions;
	if( !mvrt_io::readObj( pos[0], &vertices, &vcolors, &vemissions ) )
	{
		std::fprintf( stderr, "voxel_mesh: cannot read triangles from %s\n", pos[0] );
		return 1;
	}
	std::vector<mvrt_io::V3> otherVertices, otherColors, otherEmissions;
	if( otherObj && !mvrt_io::readObj( otherObj, &otherVertices, &otherColors, &otherEmissions ) )
	{
		std::fprintf( stderr, "voxel_mesh: cannot read triangles from %s\n", otherObj );
		return 1;
	}
	mvrt_io::V3 origin;
	float dps;
	std::vector<mvrt_io::V3> joint = vertices; // one lattice for both models
	joint.insert( joint.end(), otherVertices.begin(), otherVertices.end() );
	mvrt_io::boundingGrid( joint, gridRes, &origin, &dps );

	void* stream = nullptr;
	mvrt::IntersectorOctreeGPU svo;
	svo.build( vertices, vcolors, vemissions, nullptr, stream, origin, dps, gridRes, conservative ? MVRT_BUILD_CONSERVATIVE : 0 );
	// --fill-nearest / --solid: every enclosed cell takes the colour of its nearest voxel; `label` starts the line
	auto fillWithNearest = [&]( const char* label ) {
		const uint32_t before = svo.m_numberOfVoxels;
		uint64_t nRegions = 0, stats[8] = {};
		const uint64_t nCells = svo.enclosedNearest( 0, nullptr, nullptr, nullptr, nullptr, nullptr, &nRegions, stream );
		const uint64_t nFilled = svo.fillEnclosedNearest( stream );
		mvrt::check( mvrt_test_enclosed_nearest_stats( stats ), "mvrt_test_enclosed_nearest_stats" ); // (of the fill: the deepest squared distance)
		std::printf( "%s: voxels %u -> %u, enclosed cells %llu in %llu regions, deepest d2 %llu, filled %llu\n", label, before, svo.m_numberOfVoxels, (unsigned long long)nCells,
					 (unsigned long long)nRegions, (unsigned long long)stats[7], (unsigned long long)nFilled );
	};
	if( solid ) fillWithNearest( "solid" ); // before the second model is combined
	if( otherObj ) // before anything else is done with the octree
	{
		mvrt::IntersectorOctreeGPU other;
		other.build( otherVertices, otherColors, otherEmissions, nullptr, stream, origin, dps, gridRes, conservative ? MVRT_BUILD_CONSERVATIVE : 0 );
		mvrt::IntersectorOctreeGPU turned, *second = &other; // what is combined
		if( resampleB ) // the second set turned and scaled about the grid centre, on the same lattice
		{
			const double n = std::sqrt( rotateB[0] * rotateB[0] + rotateB[1] * rotateB[1] + rotateB[2] * rotateB[2] ), a[3] = { rotateB[0] / n, rotateB[1] / n, rotateB[2] / n };
			const double rad = rotateB[3] * 3.14159265358979323846 / 180.0, c = std::cos( rad ), sn = std::sin( rad ), t = 1.0 - c;
			const double R[9] = { c + t * a[0] * a[0],		  t * a[0] * a[1] - sn * a[2], t * a[0] * a[2] + sn * a[1], t * a[0] * a[1] + sn * a[2], c + t * a[1] * a[1],
								  t * a[1] * a[2] - sn * a[0], t * a[0] * a[2] - sn * a[1], t * a[1] * a[2] + sn * a[0], c + t * a[2] * a[2] };
			const double half = 0.5 * (double)dps * (double)gridRes, centre[3] = { (double)origin.x + half, (double)origin.y + half, (double)origin.z + half };
			double world[12]; // p' = s R ( p - centre ) + centre
			for( int i = 0; i < 3; i++ )
			{
				for( int j = 0; j < 3; j++ ) world[4 * i + j] = scaleB * R[3 * i + j];
				world[4 * i + 3] = centre[i] - ( world[4 * i] * centre[0] + world[4 * i + 1] * centre[1] + world[4 * i + 2] * centre[2] );
			}
			const mvrt::vec3 lower = { origin.x, origin.y, origin.z };
			const mvrt_cell_transform xf = mvrt::IntersectorOctreeGPU::cellTransformFromWorld( world, lower, dps, lower, dps );
			other.resample( xf, lower, dps, gridRes, 0, &turned, stream );
			std::printf( "resample-b: voxels %u -> %u, axis %g %g %g, degrees %g, scale %g\n", other.m_numberOfVoxels, turned.m_numberOfVoxels, rotateB[0], rotateB[1], rotateB[2],
						 rotateB[3], scaleB );
			second = &turned;
		}
		if( recolour ) // colour and emission of the nearest voxel of the second set
		{
			const uint64_t limit = recolourMax < 0 ? mvrt::IntersectorOctreeGPU::NO_LIMIT : (uint64_t)recolourMax * (uint64_t)recolourMax;
			uint64_t beyond = 0;
			const uint64_t changed = svo.transferAttributes( *second, offset, limit, mvrt::IntersectorOctreeGPU::TRANSFER_COLOUR | mvrt::IntersectorOctreeGPU::TRANSFER_EMISSION, &beyond,
															  stream );
			std::printf( "recolour-from: voxels %u, other %u, offset %d %d %d, max %lld, changed %llu, beyond %llu\n", svo.m_numberOfVoxels, second->m_numberOfVoxels, offset[0],
						 offset[1], offset[2], recolourMax, (unsigned long long)changed, (unsigned long long)beyond );
		}
		else if( distanceTo ) // both directions; nothing changes
		{
			const int32_t back[3] = { -offset[0], -offset[1], -offset[2] };
			const mvrt::IntersectorOctreeGPU* sets[2] = { &svo, second };
			std::printf( "distance-to: offset %d %d %d", offset[0], offset[1], offset[2] );
			for( int d = 0; d < 2; d++ ) // a -> b + o, then b + o -> a
			{
				const mvrt::IntersectorOctreeGPU::Between r =
					sets[d]->nearestBetween( *sets[1 - d], d == 0 ? offset : back, mvrt::IntersectorOctreeGPU::NO_LIMIT, 0, nullptr, nullptr, stream );
				std::vector<uint32_t> xyz, attribs;
				sets[d]->readVoxels( xyz, attribs, stream ); // (for the cell of the farthest voxel)
				std::printf( "; %s: max %.6f (d2 %llu) at voxel %u (%u %u %u), zero %llu of %llu", d == 0 ? "a -> b" : "b -> a", std::sqrt( (double)r.maxDist2 ),
							 (unsigned long long)r.maxDist2, r.farthest, xyz[3 * (size_t)r.farthest], xyz[3 * (size_t)r.farthest + 1], xyz[3 * (size_t)r.farthest + 2],
							 (unsigned long long)r.nZero, (unsigned long long)r.n );
			}
			std::printf( "\n" );
		}
		else
		{
			const uint32_t before = svo.m_numberOfVoxels, flags = attribB ? mvrt::IntersectorOctreeGPU::COMBINE_ATTRIB_B : 0u;
			uint64_t overlap = 0, clipped = 0, removed = 0;
			svo.combineVoxels( *second, combineOp, offset, flags, 0, nullptr, nullptr, nullptr, &overlap, &clipped, stream );
			const uint64_t added = svo.combine( *second, combineOp, offset, flags, &removed, nullptr, stream );
			std::printf( "%s: voxels %u -> %u, other %u, offset %d %d %d, overlap %llu, clipped %llu, added %llu, removed %llu\n", combineName, before, svo.m_numberOfVoxels,
						 second->m_numberOfVoxels, offset[0], offset[1], offset[2], (unsigned long long)overlap, (unsigned long long)clipped, (unsigned long long)added,
						 (unsigned long long)removed );
		}
	}
	if( lod > 0 ) // before anything else is done with the octree
	{
		const uint32_t before = svo.m_numberOfVoxels;
		svo.coarsen( lod, lodMinCount, 0, nullptr, stream );
		dps = svo.m_dps; // (the --ao radius is given in voxels of the mesh that is written)
		std::printf( "lod: voxels %u -> %u, gridRes %d -> %d\n", before, svo.m_numberOfVoxels, gridRes, gridRes >> lod );
	}
	if( morphOp ) // after --lod, before --fill / --exterior
	{
		const uint32_t before = svo.m_numberOfVoxels;
		uint64_t changed = 0;
		if( !std::strcmp( morphOp, "dilate" ) ) changed = svo.dilate( element, morphSteps, stream );
		else if( !std::strcmp( morphOp, "erode" ) ) changed = svo.erode( element, morphSteps, stream );
		else if( !std::strcmp( morphOp, "close" ) ) changed = svo.close( element, morphSteps, stream );
		else changed = svo.open( element, morphSteps, stream );
		std::printf( "%s: voxels %u -> %u, element %s, steps %d, %s %llu\n", morphOp, before, svo.m_numberOfVoxels, element == MVRT_MORPH_FACES ? "faces" : "cube", morphSteps,
					 !std::strcmp( morphOp, "dilate" ) || !std::strcmp( morphOp, "close" ) ? "added" : "removed", (unsigned long long)changed );
	}
	if( roundOp ) // at the same place
	{
		const uint32_t before = svo.m_numberOfVoxels, rho = (uint32_t)roundRadius2;
		uint64_t changed = 0;
		if( !std::strcmp( roundOp, "dilate" ) ) changed = svo.dilateBall( rho, stream );
		else if( !std::strcmp( roundOp, "erode" ) ) changed = svo.erodeBall( rho, stream );
		else if( !std::strcmp( roundOp, "close" ) ) changed = svo.closeBall( rho, stream );
		else changed = svo.openBall( rho, stream );
		std::printf( "round-%s: voxels %u -> %u, radius2 %u, %s %llu\n", roundOp, before, svo.m_numberOfVoxels, rho,
					 !std::strcmp( roundOp, "dilate" ) || !std::strcmp( roundOp, "close" ) ? "added" : "removed", (unsigned long long)changed );
	}
	if( components ) // what --keep-largest / --min-component select from
	{
		std::vector<uint32_t> label, size, first, box;
		svo.components( element, label, size, first, box, stream );
		std::sort( size.begin(), size.end(), []( uint32_t a, uint32_t b ) { return a > b; } );
		std::printf( "components: %zu, element %s, largest", size.size(), element == MVRT_MORPH_FACES ? "faces" : "cube" );
		for( size_t i = 0; i < size.size() && i < 5; i++ ) std::printf( " %u", size[i] );
		std::printf( "\n" );
	}
	if( keep ) // after the operators, before --fill / --exterior
	{
		const uint32_t before = svo.m_numberOfVoxels;
		const uint64_t nBefore = svo.components( element, nullptr, 0, nullptr, nullptr, nullptr, nullptr, stream );
		uint64_t nKept = 0;
		const uint64_t removed = svo.keepComponents( element, (uint64_t)minComponent, (uint32_t)keepLargest, &nKept, stream );
		std::printf( "keep: voxels %u -> %u, components %llu -> %llu, element %s, removed %llu\n", before, svo.m_numberOfVoxels, (unsigned long long)nBefore,
					 (unsigned long long)nKept, element == MVRT_MORPH_FACES ? "faces" : "cube", (unsigned long long)removed );
	}
	if( fill )
	{
		const uint32_t before = svo.m_numberOfVoxels;
		uint64_t nRegions = 0;
		const uint64_t nCells = svo.enclosedCells( 0, nullptr, nullptr, &nRegions, stream );
		const uint64_t nFilled = svo.fillEnclosed( nullptr, stream );
		std::printf( "fill: voxels %u -> %u, enclosed cells %llu in %llu regions, filled %llu\n", before, svo.m_numberOfVoxels, (unsigned long long)nCells,
					 (unsigned long long)nRegions, (unsigned long long)nFilled );
	}
	if( fillNearest ) fillWithNearest( "fill-nearest" );
	std::vector<uint32_t> xyz, attribs;
	svo.readVoxels( xyz, attribs, stream );

	std::vector<float> points;
	std::vector<uint32_t> indices, faceVoxel;
	std::vector<uint8_t> faceDir;
	uint64_t nFaces = 0, smoothClamped = 0;
	std::vector<uint8_t> masks; // --exterior: the face set of every call below
	if( exterior )
	{
		uint64_t nHidden = 0;
		const uint64_t nExterior = svo.surfaceExteriorMasks( masks, &nHidden, stream );
		std::printf( "exterior: faces %llu -> %llu, %llu look into an enclosed cell\n", (unsigned long long)( nExterior + nHidden ), (unsigned long long)nExterior,
					 (unsigned long long)nHidden );
	}
	const uint32_t mergeFlags = ( mergeAny ? MVRT_SURFACE_MERGE_ANY_ATTRIBUTE : 0u ) | ( weld ? MVRT_SURFACE_MERGE_WELD : 0u );
	if( merge )
	{
		std::vector<uint32_t> rectSize;
		nFaces = exterior ? svo.surfaceMergedMasked( masks, mergeFlags, points, indices, faceVoxel, faceDir, rectSize, stream )
						  : svo.surfaceMerged( mergeFlags, points, indices, faceVoxel, faceDir, rectSize, stream );
	}
	else if( smooth )
	{
		mvrt_smooth_params sp = mvrt::IntersectorOctreeGPU::smoothDefaultParams();
		sp.iterations = smoothIterations;
		sp.limit = smoothLimit;
		if( smoothTaubin ) sp.weightEven = 128, sp.weightOdd = -136;
		smoothClamped = exterior ? svo.surfaceSmooth( masks, sp, points, indices, faceVoxel, faceDir, stream ) : svo.surfaceSmooth( sp, points, indices, faceVoxel, faceDir, stream );
	}
	else if( weld )
	{
		if( exterior ) svo.surfaceMeshMasked( masks, points, indices, faceVoxel, faceDir, stream );
		else svo.surfaceMesh( points, indices, faceVoxel, faceDir, stream );
	}
	else if( exterior )
		svo.surfaceQuadsMasked( masks, faceVoxel, faceDir, points, stream );
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
	std::vector<uint8_t> faceRgb; // --ao: the voxel's colour scaled by the open fraction of its face
	if( ao )
	{
		std::vector<uint32_t> aoVoxel;
		std::vector<uint8_t> aoDir;
		std::vector<uint16_t> open;
		if( exterior ) svo.surfaceAoMasked( masks, aoSamples, aoRadiusVoxels * dps, aoVoxel, aoDir, open, stream );
		else svo.surfaceAo( aoSamples, aoRadiusVoxels * dps, aoVoxel, aoDir, open, stream );
		if( aoVoxel != faceVoxel || aoDir != faceDir )
		{
			std::fprintf( stderr, "voxel_mesh: the face list of the bake differs from the mesh's\n" );
			return 1;
		}
		const uint8_t* a8 = reinterpret_cast<const uint8_t*>( attribs.data() );
		faceRgb.resize( open.size() * 3 );
		for( size_t f = 0; f < open.size(); f++ )
			for( int k = 0; k < 3; k++ )
				faceRgb[f * 3 + k] = (uint8_t)( ( (uint32_t)a8[(size_t)faceVoxel[f] * 8 + k] * open[f] + (uint32_t)aoSamples / 2 ) / (uint32_t)aoSamples );
	}
	if( !mvrt_io::writePlyQuads( pos[2], points.data(), points.size() / 3, indices.data(), faceVoxel.data(), faceVoxel.size(),
								 reinterpret_cast<const uint8_t*>( attribs.data() ), ao ? faceRgb.data() : nullptr ) )
	{
		std::fprintf( stderr, "voxel_mesh: cannot write %s\n", pos[2] );
		return 1;
	}
	if( merge )
		std::printf( "voxels %u faces %llu rects %zu vertices %zu -> %s\n", svo.m_numberOfVoxels, (unsigned long long)nFaces, faceVoxel.size(), points.size() / 3, pos[2] );
	else if( smooth )
		std::printf( "voxels %u faces %zu vertices %zu smooth %d weights %d %d limit %d clamped %llu -> %s\n", svo.m_numberOfVoxels, faceVoxel.size(), points.size() / 3,
					 smoothIterations, smoothTaubin ? 128 : 256, smoothTaubin ? -136 : 256, smoothLimit, (unsigned long long)smoothClamped, pos[2] );
	else
		std::printf( "voxels %u faces %zu vertices %zu -> %s\n", svo.m_numberOfVoxels, faceVoxel.size(), points.size() / 3, pos[2] );
	return 0;
}
