// api_voxels.hip -- the C-ABI of libmvrt_hip.so (include/mvrt.h), the voxel-set operators on a built octree: surface extraction, enclosed cells and the fill,
// coarsening, morphology with the step elements and with the ball, connected components, the two-set operators and the affine resampling.  Every refusal the arguments and the handles
// decide is made here, on the host; the listings never touch the handle, the in-place calls end in adoptSorted, adoptSortedOnGrid or editHandle (api.hip).
#include "api_handles.h"

// Surface extraction (kernels_surface.hip).  Only the sorted codes and, where there is one, the cell index are read: every flavour is accepted and the
// handle is never modified.  (Builds and edits drain the steps in flight themselves; nothing here changes what a pending step reads.)
int surfaceSource( const mvrt_svo* svo, const char* who, SurfaceSource* s )
{
	REQUIRE( svo, "%s: null handle", who );
	REQUIRE( !svo->empty(), "%s: no octree (build first)", who );
	REQUIRE( svo->oct.morton.p, "%s: an uploaded octree keeps no Morton codes", who );
	const Octree& o = svo->oct;
	s->morton = o.morton.as<uint64_t>();
	s->nVoxels = o.nVoxels;
	s->levels = o.info.levels;
	s->cellBlocks = o.cellEntries.p ? o.cellBlocks.as<uint32_t>() : nullptr;
	s->cellEntries = o.cellEntries.as<uint2>();
	s->cellBits = o.cellBits;
	s->lower = mk3( o.info.lower[0], o.info.lower[1], o.info.lower[2] );
	s->dps = o.info.dps;
	s->attrs = o.attrs.as<uint2>();
	return 0;
}
MVRT_EXPORT int mvrt_svo_surface_masks( const mvrt_svo* svo, uint8_t* masksDev, uint64_t* nFacesOut, void* stream )
{
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_surface_masks", &s ) ) return 1;
	return surfaceMasks( s, masksDev, nFacesOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_surface_quads( const mvrt_svo* svo, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, uint64_t* nFacesOut,
										void* stream )
{
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_surface_quads", &s ) ) return 1;
	return surfaceQuads( s, nullptr, faceCapacity, faceVoxelDev, faceDirDev, positionsDev, nFacesOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_surface_mesh( const mvrt_svo* svo, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev,
									   float* verticesDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, void* stream )
{
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_surface_mesh", &s ) ) return 1;
	return surfaceMesh( s, nullptr, faceCapacity, vertexCapacity, faceVoxelDev, faceDirDev, indicesDev, verticesDev, nFacesOut, nVerticesOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_surface_merged( const mvrt_svo* svo, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev, uint8_t* rectDirDev,
										 uint32_t* rectSizeDev, float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut, uint64_t* nRectsOut,
										 uint64_t* nVerticesOut, void* stream )
{
	SurfaceSource s;
	if( nVerticesOut ) *nVerticesOut = 0;
	REQUIRE( ( flags & ~(uint32_t)( MVRT_SURFACE_MERGE_ANY_ATTRIBUTE | MVRT_SURFACE_MERGE_WELD ) ) == 0, "mvrt_svo_surface_merged: unknown flags 0x%x", flags );
	if( surfaceSource( svo, "mvrt_svo_surface_merged", &s ) ) return 1;
	REQUIRE( ( flags & MVRT_SURFACE_MERGE_WELD ) || ( !indicesDev && !verticesDev ), "mvrt_svo_surface_merged: indicesDev / verticesDev need MVRT_SURFACE_MERGE_WELD" );
	return surfaceMerged( s, nullptr, flags, rectCapacity, vertexCapacity, rectVoxelDev, rectDirDev, rectSizeDev, positionsDev, indicesDev, verticesDev, nFacesOut, nRectsOut, nVerticesOut,
						  (hipStream_t)stream );
}

// The same three calls on a caller's face masks, and the exterior masks as one producer of them (kernels_fill.hip).  A null handle and null masks are refused
// first, then what the namesake refuses.
MVRT_EXPORT int mvrt_svo_surface_exterior_masks( const mvrt_svo* svo, uint8_t* masksDev, uint64_t* nFacesOut, uint64_t* nHiddenOut, void* stream )
{
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_surface_exterior_masks", &s ) ) return 1;
	return surfaceExteriorMasks( s, masksDev, nFacesOut, nHiddenOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_surface_quads_masked( const mvrt_svo* svo, const uint8_t* masksDev, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev,
												 uint64_t* nFacesOut, void* stream )
{
	SurfaceSource s;
	REQUIRE( svo, "mvrt_svo_surface_quads_masked: null handle" );
	REQUIRE( masksDev, "mvrt_svo_surface_quads_masked: null masksDev" );
	if( surfaceSource( svo, "mvrt_svo_surface_quads_masked", &s ) ) return 1;
	return surfaceQuads( s, masksDev, faceCapacity, faceVoxelDev, faceDirDev, positionsDev, nFacesOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_surface_mesh_masked( const mvrt_svo* svo, const uint8_t* masksDev, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev,
												uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, void* stream )
{
	SurfaceSource s;
	REQUIRE( svo, "mvrt_svo_surface_mesh_masked: null handle" );
	REQUIRE( masksDev, "mvrt_svo_surface_mesh_masked: null masksDev" );
	if( surfaceSource( svo, "mvrt_svo_surface_mesh_masked", &s ) ) return 1;
	return surfaceMesh( s, masksDev, faceCapacity, vertexCapacity, faceVoxelDev, faceDirDev, indicesDev, verticesDev, nFacesOut, nVerticesOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_surface_merged_masked( const mvrt_svo* svo, const uint8_t* masksDev, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev,
												  uint8_t* rectDirDev, uint32_t* rectSizeDev, float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut,
												  uint64_t* nRectsOut, uint64_t* nVerticesOut, void* stream )
{
	SurfaceSource s;
	if( nVerticesOut ) *nVerticesOut = 0;
	REQUIRE( ( flags & ~(uint32_t)( MVRT_SURFACE_MERGE_ANY_ATTRIBUTE | MVRT_SURFACE_MERGE_WELD ) ) == 0, "mvrt_svo_surface_merged_masked: unknown flags 0x%x", flags );
	REQUIRE( svo, "mvrt_svo_surface_merged_masked: null handle" );
	REQUIRE( masksDev, "mvrt_svo_surface_merged_masked: null masksDev" );
	if( surfaceSource( svo, "mvrt_svo_surface_merged_masked", &s ) ) return 1;
	REQUIRE( ( flags & MVRT_SURFACE_MERGE_WELD ) || ( !indicesDev && !verticesDev ), "mvrt_svo_surface_merged_masked: indicesDev / verticesDev need MVRT_SURFACE_MERGE_WELD" );
	return surfaceMerged( s, masksDev, flags, rectCapacity, vertexCapacity, rectVoxelDev, rectDirDev, rectSizeDev, positionsDev, indicesDev, verticesDev, nFacesOut, nRectsOut,
						  nVerticesOut, (hipStream_t)stream );
}

// Constrained surface nets (kernels_smooth.hip).  The parameters are looked at before the handle: a bad field is named whatever the handle holds.
MVRT_EXPORT int mvrt_smooth_default_params( mvrt_smooth_params* p )
{
	REQUIRE( p, "mvrt_smooth_default_params: null argument" );
	memset( p, 0, sizeof( *p ) );
	p->iterations = 4;
	p->weightEven = p->weightOdd = 256;
	p->limit = 127;
	return 0;
}
MVRT_EXPORT int mvrt_svo_surface_smooth( const mvrt_svo* svo, const uint8_t* masksDev, const mvrt_smooth_params* params, uint64_t faceCapacity, uint64_t vertexCapacity,
										 uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev, float* verticesDev, int32_t* displacementsDev, uint8_t* neighboursDev,
										 uint64_t* nFacesOut, uint64_t* nVerticesOut, uint64_t* clampedOut, void* stream )
{
	const char* who = "mvrt_svo_surface_smooth";
	mvrt_smooth_params p;
	mvrt_smooth_default_params( &p );
	if( params ) p = *params;
	REQUIRE( svo, "%s: null handle", who );
	REQUIRE( p.iterations >= 0 && p.iterations <= 256, "%s: iterations %d outside 0..256", who, p.iterations );
	REQUIRE( p.weightEven >= -256 && p.weightEven <= 256, "%s: weightEven %d outside -256..256", who, p.weightEven );
	REQUIRE( p.weightOdd >= -256 && p.weightOdd <= 256, "%s: weightOdd %d outside -256..256", who, p.weightOdd );
	REQUIRE( p.limit >= 0 && p.limit <= 128, "%s: limit %d outside 0..128", who, p.limit );
	for( int k = 0; k < 4; k++ ) REQUIRE( p.reserved[k] == 0, "%s: reserved[%d] is 0x%x, not 0", who, k, p.reserved[k] );
	SurfaceSource s;
	if( surfaceSource( svo, who, &s ) ) return 1;
	const SmoothRule rule = { p.iterations, p.weightEven, p.weightOdd, p.limit };
	return surfaceSmooth( s, masksDev, rule, faceCapacity, vertexCapacity, faceVoxelDev, faceDirDev, indicesDev, verticesDev, displacementsDev, neighboursDev, nFacesOut, nVerticesOut,
						  clampedOut, (hipStream_t)stream );
}

// Enclosed empty cells and the fill (kernels_fill.hip).  The listing reads the sorted codes alone, like the surface calls.  The fill hands the cells, which stay on
// the device, to the edit's own route (editHandle, api.hip): what it leaves is what mvrt_svo_edit_voxels leaves, by construction.
MVRT_EXPORT int mvrt_svo_enclosed_cells( const mvrt_svo* svo, uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint64_t* nCellsOut, uint64_t* nRegionsOut, void* stream )
{
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_enclosed_cells", &s ) ) return 1;
	return enclosedCells( s, capacity, xyzDev, regionDev, nCellsOut, nRegionsOut, (hipStream_t)stream );
}
// both fills: they differ in the step that makes the cells, which for the nearest-voxel fill brings one attribute per cell along (fillAttribHost is null then)
static int fillEnclosed( mvrt_svo* svo, const char* who, bool nearest, const uint8_t* fillAttribHost, uint64_t* nFilledOut, void* stream )
{
	if( nFilledOut ) *nFilledOut = 0;
	SurfaceSource s;
	if( surfaceSource( svo, who, &s ) ) return 1;
	hipStream_t st = (hipStream_t)stream;
	DevBuf xyz, attribs;
	uint64_t nCells = 0;
	if( nearest ? enclosedNearestUnordered( s, xyz, attribs, &nCells, st ) : enclosedCellsUnordered( s, xyz, &nCells, st ) ) return 1; // (near is taken on the set as it is now)
	if( nCells == 0 ) return 0; // nothing to fill: the handle is not touched
	REQUIRE( (uint64_t)svo->oct.nVoxels + nCells < 0xFFFFFFFFull, "%s: %llu voxels and %llu enclosed cells exceed the 32-bit index range of the builder", who,
			 (unsigned long long)svo->oct.nVoxels, (unsigned long long)nCells );
	if( fillAttribHost )
	{
		uint2 a;
		memcpy( &a, fillAttribHost, 8 );
		if( attribs.alloc( nCells * 8 ) || launchFillAttribs( a, nCells, attribs.as<uint2>(), st ) ) return 1;
	}
	if( editHandle( svo, who, EDIT_STRUCTURAL, xyz.as<uint32_t>(), attribs.as<uint32_t>(), nullptr, nCells, &xyz, &attribs, st ) ) return 1;
	if( nFilledOut ) *nFilledOut = nCells;
	return 0;
}
MVRT_EXPORT int mvrt_svo_fill_enclosed( mvrt_svo* svo, const uint8_t fillAttribHost[8], uint64_t* nFilledOut, void* stream )
{
	return fillEnclosed( svo, "mvrt_svo_fill_enclosed", false, fillAttribHost, nFilledOut, stream );
}

// The same cells with their nearest voxel, and the fill that takes its colours from them (kernels_nearest.hip).  The fill is mvrt_svo_fill_enclosed with one
// attribute per cell: the same function (fillEnclosed above), so the same route through the edit and the same refusals in the same order.
MVRT_EXPORT int mvrt_svo_enclosed_nearest( const mvrt_svo* svo, uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev,
										   uint64_t* nCellsOut, uint64_t* nRegionsOut, void* stream )
{
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_enclosed_nearest", &s ) ) return 1;
	return enclosedNearest( s, capacity, xyzDev, regionDev, dist2Dev, nearestDev, attribsDev, nCellsOut, nRegionsOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_fill_enclosed_nearest( mvrt_svo* svo, uint64_t* nFilledOut, void* stream )
{
	return fillEnclosed( svo, "mvrt_svo_fill_enclosed_nearest", true, nullptr, nFilledOut, stream );
}
MVRT_EXPORT int mvrt_test_enclosed_nearest_stats( uint64_t out[8] )
{
	const NearestStats t = nearestLastStats();
	REQUIRE( out, "mvrt_test_enclosed_nearest_stats: null out" );
	out[0] = t.cells;
	for( int k = 0; k < 3; k++ ) out[1 + k] = t.gaps[k], out[4 + k] = t.longest[k];
	out[7] = t.deepest;
	return 0;
}

// A coarser level of detail (kernels_coarsen.hip).  Every refusal is made here, on the host: first what the arguments alone decide, then the handle.  The listing
// reads the sorted codes and the attributes alone; the build hands the list, which stays on the device, to the levels of the voxel-list build.
static int coarsenSource( const mvrt_svo* svo, const char* who, int levelsDown, uint64_t minCount )
{
	REQUIRE( levelsDown >= 1 && levelsDown <= 20, "%s: levelsDown %d is outside [1, log2( gridRes ) - 1] (20 at most, for gridRes 2^21)", who, levelsDown );
	REQUIRE( minCount >= 1 && minCount <= coarseCellCapacity( levelsDown ), "%s: minCount %llu is outside [1, 8^levelsDown = %llu]", who, (unsigned long long)minCount,
			 (unsigned long long)coarseCellCapacity( levelsDown ) );
	REQUIRE( !svo->empty(), "%s: no octree (build first)", who );
	REQUIRE( svo->oct.morton.p, "%s: an uploaded octree keeps no Morton codes", who );
	const int L = (int)svo->oct.info.levels;
	REQUIRE( levelsDown <= L - 1, "%s: levelsDown %d is outside [1, %d] = [1, log2( gridRes ) - 1] for gridRes %u", who, levelsDown, L - 1, svo->oct.info.gridRes );
	return 0;
}
MVRT_EXPORT int mvrt_svo_coarse_voxels( const mvrt_svo* svo, int levelsDown, uint64_t minCount, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* countDev,
										uint64_t* nOut, void* stream )
{
	REQUIRE( svo, "mvrt_svo_coarse_voxels: null handle" );
	if( coarsenSource( svo, "mvrt_svo_coarse_voxels", levelsDown, minCount ) ) return 1;
	const Octree& o = svo->oct;
	return coarseVoxels( o.morton.as<uint64_t>(), o.attrs.as<uint2>(), o.nVoxels, levelsDown, minCount, capacity, xyzDev, attribsDev, countDev, nOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_coarsen( const mvrt_svo* src, mvrt_svo* dst, int levelsDown, uint64_t minCount, int buildFlags, void* stream )
{
	REQUIRE( src && dst, "mvrt_svo_coarsen: null handle" );
	REQUIRE_BUILD_FLAGS( "mvrt_svo_coarsen", buildFlags );
	if( coarsenSource( src, "mvrt_svo_coarsen", levelsDown, minCount ) ) return 1;
	const mvrt_svo_info info = src->oct.info; // (a copy: dst may be src)
	const float dps = info.dps * (float)( 1u << levelsDown ); // exact: a power of two
	REQUIRE( dps - dps == 0.0f, "mvrt_svo_coarsen: dps %g times 2^%d is not finite", (double)info.dps, levelsDown );
	const int gridRes = (int)( info.gridRes >> levelsDown );
	const uint32_t nFine = src->oct.nVoxels;
	hipStream_t st = (hipStream_t)stream;
	if( ownerDrain( dst ) ) return 1; // steps already issued render the old scene
	SortedVoxels v;
	if( coarseList( src->oct.morton.as<uint64_t>(), src->oct.attrs.as<uint2>(), nFine, levelsDown, minCount, v, st ) ) return 1;
	REQUIRE( v.n >= 1, "mvrt_svo_coarsen: minCount %llu would leave no voxel (no coarse cell holds that many of the %u voxels)", (unsigned long long)minCount, nFine );
	return adoptSortedOnGrid( dst, v, nFine, info.lower, dps, gridRes, buildFlags, nullptr, st ); // (the source is read before the old octree of dst goes)
}

// The attribute pyramid of the cone-limited rays (kernels_lod.hip): the listing above once per level, kept with the handle.  The refusals are the listing's, with its
// words, then the two of the device view the pyramid is read through.  The old pyramid goes first; the new one is moved in whole or not at all
MVRT_EXPORT int mvrt_svo_lod_prepare( mvrt_svo* svo, void* stream )
{
	REQUIRE( svo, "mvrt_svo_lod_prepare: null handle" );
	REQUIRE( !svo->empty(), "mvrt_svo_lod_prepare: no octree (build first)" );
	REQUIRE( svo->oct.morton.p, "mvrt_svo_lod_prepare: an uploaded octree keeps no Morton codes" );
	REQUIRE( !svo->oct.tree, "mvrt_svo_lod_prepare: tree-flavour octrees (MVRT_FLAVOUR_TREE) are not supported" );
	REQUIRE( svo->oct.info.levels <= MVRT_DEVICE_MAX_LEVELS, "mvrt_svo_lod_prepare: %u levels, the device API supports at most %d", svo->oct.info.levels, MVRT_DEVICE_MAX_LEVELS );
	Octree& o = svo->oct;
	o.lod = LodPyramid();
	return lodBuild( o.morton.as<uint64_t>(), o.attrs.as<uint2>(), o.nVoxels, o.info.levels, &o.lod, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_lod_release( mvrt_svo* svo )
{
	REQUIRE( svo, "mvrt_svo_lod_release: null handle" );
	svo->oct.lod = LodPyramid();
	return 0;
}
MVRT_EXPORT uint64_t mvrt_svo_lod_bytes( const mvrt_svo* svo ) { return svo && svo->oct.lod.ready ? svo->oct.lod.bytes() : 0; }
MVRT_EXPORT int mvrt_svo_lod_view( const mvrt_svo* svo, mvrt_device_lod* out )
{
	REQUIRE( svo && out, "mvrt_svo_lod_view: null argument" );
	REQUIRE( !svo->empty(), "mvrt_svo_lod_view: no octree (build first)" );
	const Octree& o = svo->oct;
	REQUIRE( o.lod.ready, "mvrt_svo_lod_view: no attribute pyramid (mvrt_svo_lod_prepare first)" );
	mvrt_device_lod v;
	memset( &v, 0, sizeof( v ) );
	v.structBytes = sizeof( mvrt_device_lod );
	v.levels = o.info.levels;
	for( uint32_t L = 1; L < o.info.levels; L++ )
	{
		v.codes[L] = (uint64_t)(uintptr_t)o.lod.codes[L].p;
		v.attrs[L] = (uint64_t)(uintptr_t)o.lod.attrs[L].p;
		v.cellVoxels[L] = (uint64_t)(uintptr_t)o.lod.counts[L].p;
		v.count[L] = o.lod.n[L];
	}
	v.codes[o.info.levels] = (uint64_t)(uintptr_t)o.morton.p; // the last level is the voxel list itself: the rank is the vIndex
	v.attrs[o.info.levels] = (uint64_t)(uintptr_t)o.attrs.p;
	v.count[o.info.levels] = o.nVoxels;
	*out = v;
	return 0;
}

// Dilation, erosion, closing and opening (kernels_morph.hip).  Every refusal the arguments and the handle decide is made here, on the host.  The listings read the
// sorted codes and the attributes alone; the in-place calls run their steps on sorted lists next to the old octree and build the levels once, from the last list.
static int morphSource( const mvrt_svo* svo, const char* who, int element, SurfaceSource* s )
{
	if( surfaceSource( svo, who, s ) ) return 1;
	REQUIRE( element == MVRT_MORPH_FACES || element == MVRT_MORPH_CUBE, "%s: unknown element %d (MVRT_MORPH_FACES = 0, MVRT_MORPH_CUBE = 1)", who, element );
	return 0;
}
MVRT_EXPORT int mvrt_svo_dilation_cells( const mvrt_svo* svo, int element, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* countDev, uint64_t* nOut,
										 void* stream )
{
	SurfaceSource s;
	if( morphSource( svo, "mvrt_svo_dilation_cells", element, &s ) ) return 1;
	return morphDilationCells( s, element, capacity, xyzDev, attribsDev, countDev, nOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_erosion_voxels( const mvrt_svo* svo, int element, uint64_t capacity, uint32_t* vIndexDev, uint64_t* nOut, void* stream )
{
	SurfaceSource s;
	if( morphSource( svo, "mvrt_svo_erosion_voxels", element, &s ) ) return 1;
	return morphErosionVoxels( s, element, capacity, vIndexDev, nOut, (hipStream_t)stream );
}
// the out-count of the morphological in-place calls: the voxels added or removed (0, as preset, when nothing changed)
static void countChange( uint32_t nOld, uint32_t n, uint64_t* nChangedOut )
{
	if( nChangedOut ) *nChangedOut = n > nOld ? n - nOld : nOld - n;
}
static int morphInPlace( mvrt_svo* svo, const char* who, int op, int element, int steps, uint64_t* nChangedOut, void* stream )
{
	if( nChangedOut ) *nChangedOut = 0;
	SurfaceSource s;
	if( morphSource( svo, who, element, &s ) ) return 1;
	REQUIRE( steps >= 1 && steps <= 64, "%s: steps %d is outside [1, 64]", who, steps );
	hipStream_t st = (hipStream_t)stream;
	SortedVoxels v;
	if( morphList( who, s, element, op, steps, v, st ) || adoptSorted( svo, v, st ) ) return 1;
	countChange( s.nVoxels, v.n, nChangedOut );
	return 0;
}
MVRT_EXPORT int mvrt_svo_dilate( mvrt_svo* svo, int element, int steps, uint64_t* nAddedOut, void* stream )
{
	return morphInPlace( svo, "mvrt_svo_dilate", MVRT_MORPH_OP_DILATE, element, steps, nAddedOut, stream );
}
MVRT_EXPORT int mvrt_svo_erode( mvrt_svo* svo, int element, int steps, uint64_t* nRemovedOut, void* stream )
{
	return morphInPlace( svo, "mvrt_svo_erode", MVRT_MORPH_OP_ERODE, element, steps, nRemovedOut, stream );
}
MVRT_EXPORT int mvrt_svo_close( mvrt_svo* svo, int element, int steps, uint64_t* nAddedOut, void* stream )
{
	return morphInPlace( svo, "mvrt_svo_close", MVRT_MORPH_OP_CLOSE, element, steps, nAddedOut, stream );
}
MVRT_EXPORT int mvrt_svo_open( mvrt_svo* svo, int element, int steps, uint64_t* nRemovedOut, void* stream )
{
	return morphInPlace( svo, "mvrt_svo_open", MVRT_MORPH_OP_OPEN, element, steps, nRemovedOut, stream );
}

// Round offsets (kernels_ball.hip).  Every refusal the arguments and the handle decide is made here, on the host.  The listings read the sorted codes and the
// attributes alone; the in-place calls run their halves on sorted lists next to the old octree and build the levels once, as the morphology above does.
static int ballSource( const mvrt_svo* svo, const char* who, uint32_t radius2, SurfaceSource* s )
{
	if( surfaceSource( svo, who, s ) ) return 1;
	REQUIRE( radius2 >= 1u && radius2 <= 1024u, "%s: radius2 %u is outside [1, 1024]", who, radius2 );
	return 0;
}
MVRT_EXPORT int mvrt_svo_distance_cells( const mvrt_svo* svo, uint32_t radius2, uint64_t capacity, uint32_t* xyzDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev,
										 uint64_t* nOut, void* stream )
{
	SurfaceSource s;
	if( ballSource( svo, "mvrt_svo_distance_cells", radius2, &s ) ) return 1;
	return ballDistanceCells( s, radius2, capacity, xyzDev, dist2Dev, nearestDev, attribsDev, nOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_depth_voxels( const mvrt_svo* svo, uint32_t radius2, uint64_t capacity, uint32_t* vIndexDev, uint32_t* depth2Dev, uint64_t* nOut, void* stream )
{
	SurfaceSource s;
	if( ballSource( svo, "mvrt_svo_depth_voxels", radius2, &s ) ) return 1;
	return ballDepthVoxels( s, radius2, capacity, vIndexDev, depth2Dev, nOut, (hipStream_t)stream );
}
static int ballInPlace( mvrt_svo* svo, const char* who, int op, uint32_t radius2, uint64_t* nChangedOut, void* stream )
{
	if( nChangedOut ) *nChangedOut = 0;
	SurfaceSource s;
	if( ballSource( svo, who, radius2, &s ) ) return 1;
	hipStream_t st = (hipStream_t)stream;
	SortedVoxels v;
	if( ballList( who, s, radius2, op, v, st ) || adoptSorted( svo, v, st ) ) return 1;
	countChange( s.nVoxels, v.n, nChangedOut );
	return 0;
}
MVRT_EXPORT int mvrt_svo_dilate_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nAddedOut, void* stream )
{
	return ballInPlace( svo, "mvrt_svo_dilate_ball", MVRT_MORPH_OP_DILATE, radius2, nAddedOut, stream );
}
MVRT_EXPORT int mvrt_svo_erode_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nRemovedOut, void* stream )
{
	return ballInPlace( svo, "mvrt_svo_erode_ball", MVRT_MORPH_OP_ERODE, radius2, nRemovedOut, stream );
}
MVRT_EXPORT int mvrt_svo_close_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nAddedOut, void* stream )
{
	return ballInPlace( svo, "mvrt_svo_close_ball", MVRT_MORPH_OP_CLOSE, radius2, nAddedOut, stream );
}
MVRT_EXPORT int mvrt_svo_open_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nRemovedOut, void* stream )
{
	return ballInPlace( svo, "mvrt_svo_open_ball", MVRT_MORPH_OP_OPEN, radius2, nRemovedOut, stream );
}
MVRT_EXPORT int mvrt_test_peak_bytes( uint64_t* peakOut, int reset )
{
	if( peakOut ) *peakOut = g_devBufState.peakBytes;
	if( reset ) g_devBufState.peakBytes = g_devBufState.liveBytes.load();
	return 0;
}
MVRT_EXPORT int mvrt_test_ball_stats( uint64_t out[5] )
{
	const BallStats b = ballLastStats();
	REQUIRE( out, "mvrt_test_ball_stats: null out" );
	for( int k = 0; k < 3; k++ ) out[k] = b.records[k];
	out[3] = b.seeds;
	out[4] = b.cells;
	return 0;
}

// Connected components (kernels_components.hip).  Every refusal the arguments and the handle decide is made here, on the host.  The listing reads the sorted codes
// alone; the in-place call compacts the kept voxels next to the old octree and builds the levels once, as the opening does.  The handle and the element are
// checked by morphSource: the connectivity is a structuring element.
MVRT_EXPORT int mvrt_svo_components( const mvrt_svo* svo, int element, uint32_t* labelDev, uint64_t componentCapacity, uint32_t* sizeDev, uint32_t* firstDev, uint32_t* boxDev,
									 uint64_t* nComponentsOut, uint64_t* largestOut, void* stream )
{
	SurfaceSource s;
	if( morphSource( svo, "mvrt_svo_components", element, &s ) ) return 1;
	return componentsList( s, element, labelDev, componentCapacity, sizeDev, firstDev, boxDev, nComponentsOut, largestOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_keep_components( mvrt_svo* svo, int element, uint64_t minVoxels, uint32_t keepLargest, uint64_t* nRemovedOut, uint64_t* nKeptOut, void* stream )
{
	const char* who = "mvrt_svo_keep_components";
	if( nRemovedOut ) *nRemovedOut = 0;
	if( nKeptOut ) *nKeptOut = 0;
	SurfaceSource s;
	if( morphSource( svo, who, element, &s ) ) return 1;
	REQUIRE( minVoxels >= 1, "%s: minVoxels 0 (1 keeps every component)", who );
	hipStream_t st = (hipStream_t)stream;
	SortedVoxels v;
	uint32_t nComponents = 0, nKept = 0;
	if( componentsKeepList( s, element, minVoxels, keepLargest, v, &nComponents, &nKept, st ) ) return 1;
	REQUIRE( nKept >= 1, "%s: minVoxels %llu would leave no voxel (the largest of the %u components is smaller)", who, (unsigned long long)minVoxels, nComponents );
	if( adoptSorted( svo, v, st ) ) return 1; // (every component kept: the list is unchanged and the handle is not touched)
	if( nRemovedOut ) *nRemovedOut = s.nVoxels - v.n;
	if( nKeptOut ) *nKeptOut = nKept;
	return 0;
}

// Two voxel sets (kernels_combine.hip).  Every refusal the arguments and the handles decide is made here, on the host.  The listing reads the sorted codes and the
// attributes of both handles; the in-place call emits the result next to the old octree and builds the levels once, as the opening does.
static_assert( MVRT_COMBINE_UNION == MVRT_COMBINE_OP_UNION && MVRT_COMBINE_INTERSECTION == MVRT_COMBINE_OP_INTERSECTION && MVRT_COMBINE_DIFFERENCE == MVRT_COMBINE_OP_DIFFERENCE &&
				   MVRT_COMBINE_XOR == MVRT_COMBINE_OP_XOR && (int)MVRT_COMBINE_ATTRIB_B == MVRT_COMBINE_FLAG_ATTRIB_B,
			   "mvrt.h and launch.h number the operators alike" );
// The second handle of a two-set call, in the words of the call (`missing`: how it names one that is not there, `name`: how it names the handle), and its cell offset: the
// checks of the two-set operators here and of the nearest-voxel calls below
static int secondSource( const mvrt_svo* b, const char* who, const char* missing, const char* name, SurfaceSource* sb )
{
	REQUIRE( b, "%s: null %s", who, missing );
	REQUIRE( !b->empty(), "%s: %s holds no octree (build first)", who, name );
	REQUIRE( b->oct.morton.p, "%s: %s is an uploaded octree, which keeps no Morton codes", who, name );
	return surfaceSource( b, who, sb );
}
static int cellOffset( const char* who, const int32_t offset[3], int32_t o[3] )
{
	for( int k = 0; k < 3; k++ )
	{
		o[k] = offset ? offset[k] : 0;
		REQUIRE( o[k] >= -( 1 << 21 ) && o[k] <= ( 1 << 21 ), "%s: offset[%d] = %d is outside [-2^21, 2^21]", who, k, o[k] );
	}
	return 0;
}
static int combineSources( const mvrt_svo* a, const mvrt_svo* b, const char* who, int op, const int32_t offset[3], uint32_t flags, SurfaceSource* sa, SurfaceSource* sb, int32_t o[3] )
{
	if( surfaceSource( a, who, sa ) || secondSource( b, who, "handle b", "b", sb ) ) return 1;
	REQUIRE( op >= MVRT_COMBINE_UNION && op <= MVRT_COMBINE_XOR, "%s: unknown op %d (MVRT_COMBINE_UNION = 0, _INTERSECTION = 1, _DIFFERENCE = 2, _XOR = 3)", who, op );
	REQUIRE( ( flags & ~(uint32_t)MVRT_COMBINE_ATTRIB_B ) == 0, "%s: unknown flags 0x%x (MVRT_COMBINE_ATTRIB_B only)", who, flags );
	return cellOffset( who, offset, o );
}
MVRT_EXPORT int mvrt_svo_combine_voxels( const mvrt_svo* a, const mvrt_svo* b, int op, const int32_t offset[3], uint32_t flags, uint64_t capacity, uint32_t* xyzDev,
										 uint32_t* attribsDev, uint8_t* sourceDev, uint64_t* nOut, uint64_t* nOverlapOut, uint64_t* nClippedOut, void* stream )
{
	SurfaceSource sa, sb;
	int32_t o[3];
	if( combineSources( a, b, "mvrt_svo_combine_voxels", op, offset, flags, &sa, &sb, o ) ) return 1;
	return combineVoxels( sa, sb, op, o, flags, capacity, xyzDev, attribsDev, sourceDev, nOut, nOverlapOut, nClippedOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_combine( mvrt_svo* a, const mvrt_svo* b, int op, const int32_t offset[3], uint32_t flags, uint64_t* nAddedOut, uint64_t* nRemovedOut,
								  uint64_t* nClippedOut, void* stream )
{
	const char* who = "mvrt_svo_combine";
	if( nAddedOut ) *nAddedOut = 0;
	if( nRemovedOut ) *nRemovedOut = 0;
	if( nClippedOut ) *nClippedOut = 0;
	SurfaceSource sa, sb;
	int32_t o[3];
	if( combineSources( a, b, who, op, offset, flags, &sa, &sb, o ) ) return 1;
	hipStream_t st = (hipStream_t)stream;
	CombineCounts c;
	if( combineList( who, sa, sb, op, o, flags, &c, st ) ) return 1;
	if( nClippedOut ) *nClippedOut = c.nClipped;
	if( c.nAdded == 0 && c.nRemoved == 0 ) // the node structure stays
	{
		if( !c.recolours ) return 0; // nothing changes: the handle is not touched
		if( ownerDrain( a ) ) return 1; // steps already issued render the old scene; a recolouring writes in place
		a->oct.lod = LodPyramid();		// (as editHandle: the pyramid's means are of the colours about to go)
		MVRT_HIP( hipMemcpyAsync( a->oct.attrs.p, c.list.attrs.p, (uint64_t)c.list.n * 8, hipMemcpyDeviceToDevice, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
		a->oct.totalDumped = 0;
		a->oct.hasEmission = c.list.hasEmission;
		return 0;
	}
	if( adoptSorted( a, c.list, st ) ) return 1; // (b == a was read above)
	if( nAddedOut ) *nAddedOut = c.nAdded;
	if( nRemovedOut ) *nRemovedOut = c.nRemoved;
	return 0;
}

// The nearest voxel of arbitrary lattice points (kernels_query.hip).  Every refusal the arguments and the handles decide is made here, on the host.  The listings
// never touch a handle; the transfer hands its list, which stays on the device, to the edit's own attribute-only path, as the fills do.
static_assert( MVRT_TRANSFER_COLOUR == 1u && MVRT_TRANSFER_EMISSION == 2u, "mvrt.h and nearestTransferAttrib number the words alike" );
static int querySources( const mvrt_svo* a, const mvrt_svo* b, const char* who, const int32_t offset[3], SurfaceSource* sa, SurfaceSource* sb, int32_t o[3] )
{
	return surfaceSource( a, who, sa ) || secondSource( b, who, "second handle", "the second handle", sb ) || cellOffset( who, offset, o );
}
MVRT_EXPORT int mvrt_svo_nearest_voxels( const mvrt_svo* svo, uint64_t n, const int32_t* queryDev, uint64_t maxDist2, uint64_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev,
										 void* stream )
{
	const char* who = "mvrt_svo_nearest_voxels";
	SurfaceSource s;
	if( surfaceSource( svo, who, &s ) ) return 1;
	REQUIRE( n < ( 1ull << 32 ), "%s: %llu queries are 2^32 or more", who, (unsigned long long)n );
	REQUIRE( n == 0 || queryDev, "%s: null queries", who );
	return nearestVoxels( s, n, queryDev, maxDist2, dist2Dev, nearestDev, attribsDev, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_nearest_between( const mvrt_svo* a, const mvrt_svo* b, const int32_t offset[3], uint64_t maxDist2, uint64_t capacity, uint64_t* dist2Dev, uint32_t* nearestDev,
										  uint64_t* nOut, uint64_t* maxDist2Out, uint32_t* farthestOut, uint64_t* nZeroOut, uint64_t* nBeyondOut, void* stream )
{
	if( nOut ) *nOut = 0;
	SurfaceSource sa, sb;
	int32_t o[3];
	if( querySources( a, b, "mvrt_svo_nearest_between", offset, &sa, &sb, o ) ) return 1;
	NearestBetweenCounts c;
	const int rc = nearestBetween( sa, sb, o, maxDist2, capacity, dist2Dev, nearestDev, &c, (hipStream_t)stream );
	if( nOut ) *nOut = c.n; // (still returned where the capacity is refused)
	if( rc ) return 1;
	if( maxDist2Out ) *maxDist2Out = c.maxDist2;
	if( farthestOut ) *farthestOut = c.farthest;
	if( nZeroOut ) *nZeroOut = c.nZero;
	if( nBeyondOut ) *nBeyondOut = c.nBeyond;
	return 0;
}
MVRT_EXPORT int mvrt_svo_transfer_attributes( mvrt_svo* dst, const mvrt_svo* src, const int32_t offset[3], uint64_t maxDist2, uint32_t flags, uint64_t* nChangedOut,
											  uint64_t* nBeyondOut, void* stream )
{
	const char* who = "mvrt_svo_transfer_attributes";
	if( nChangedOut ) *nChangedOut = 0;
	if( nBeyondOut ) *nBeyondOut = 0;
	SurfaceSource sd, ss;
	int32_t o[3];
	if( querySources( dst, src, who, offset, &sd, &ss, o ) ) return 1;
	REQUIRE( flags != 0u && ( flags & ~( MVRT_TRANSFER_COLOUR | MVRT_TRANSFER_EMISSION ) ) == 0u, "%s: flags 0x%x are not MVRT_TRANSFER_COLOUR (1) | MVRT_TRANSFER_EMISSION (2)",
			 who, flags );
	hipStream_t st = (hipStream_t)stream;
	DevBuf xyz, attribs;
	uint64_t nTaken = 0, nChanged = 0, nBeyond = 0;
	if( nearestTransferList( sd, ss, o, maxDist2, flags, xyz, attribs, &nTaken, &nChanged, &nBeyond, st ) ) return 1; // (near is taken in src as it is now)
	if( nBeyondOut ) *nBeyondOut = nBeyond;
	if( nChanged == 0 ) return 0; // no byte changes: the handle is not touched
	if( editHandle( dst, who, EDIT_ATTRIBUTES, xyz.as<uint32_t>(), attribs.as<uint32_t>(), nullptr, nTaken, nullptr, nullptr, st ) ) return 1; // (every entry is a voxel of dst)
	if( nChangedOut ) *nChangedOut = nChanged;
	return 0;
}
MVRT_EXPORT int mvrt_test_nearest_query_stats( uint64_t out[4] )
{
	const NearestQueryStats t = nearestQueryLastStats();
	REQUIRE( out, "mvrt_test_nearest_query_stats: null out" );
	out[0] = t.queries, out[1] = t.visits, out[2] = t.mostVisits, out[3] = t.compared;
	return 0;
}

// Affine resampling (kernels_resample.hip).  Every refusal the arguments and the handles decide is made here, on the host: first what the arguments alone decide
// (a null handle, the transform, the grid), then the handle, as the coarsening does.  The listing reads the sorted codes and the attributes alone; the build hands the list, which stays on the device, to the
// levels of the voxel-list build, as the coarsening does.
static_assert( MVRT_TRANSFORM_FRAC_BITS == 24 && sizeof( mvrt_cell_transform ) == 8 + 12 * 8, "mvrt.h and kernels_resample.hip agree on the fixed point and the record" );
static int resampleSource( const mvrt_svo* src, const char* who, const mvrt_cell_transform* xf, int dstGridRes, SurfaceSource* s )
{
	REQUIRE( src, "%s: null handle", who );
	REQUIRE( xf, "%s: null transform", who );
	REQUIRE( xf->structBytes == sizeof( mvrt_cell_transform ), "%s: structBytes %u is not sizeof( mvrt_cell_transform ) = %u", who, xf->structBytes,
			 (unsigned)sizeof( mvrt_cell_transform ) );
	REQUIRE( xf->reserved == 0u, "%s: the reserved field of the transform is %u, not 0", who, xf->reserved );
	REQUIRE( resampleTransformValid( xf->m, xf->t ), "%s: an entry of the transform is out of range (|m[k]| <= 2^30, |t[i]| <= 2^52)", who );
	REQUIRE( levelsOf( dstGridRes ) > 0 && dstGridRes <= ( 1 << 21 ), "%s: dstGridRes %d is not a power of two in [2, 2^21]", who, dstGridRes );
	return surfaceSource( src, who, s );
}
MVRT_EXPORT int mvrt_svo_resample_voxels( const mvrt_svo* src, const mvrt_cell_transform* xf, int dstGridRes, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev,
										  uint32_t* sourceDev, uint64_t* nOut, void* stream )
{
	SurfaceSource s;
	if( resampleSource( src, "mvrt_svo_resample_voxels", xf, dstGridRes, &s ) ) return 1;
	return resampleVoxels( s, xf->m, xf->t, (uint32_t)levelsOf( dstGridRes ), capacity, xyzDev, attribsDev, sourceDev, nOut, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_resample( const mvrt_svo* src, mvrt_svo* dst, const mvrt_cell_transform* xf, const float dstOriginHost[3], float dstDps, int dstGridRes, int buildFlags,
								   uint64_t* nOut, void* stream )
{
	const char* who = "mvrt_svo_resample";
	if( nOut ) *nOut = 0;
	REQUIRE( src && dst, "%s: null handle", who );
	REQUIRE_BUILD_FLAGS( who, buildFlags );
	SurfaceSource s;
	if( resampleSource( src, who, xf, dstGridRes, &s ) ) return 1;
	REQUIRE( dstOriginHost, "%s: null origin", who );
	const float origin[3] = { dstOriginHost[0], dstOriginHost[1], dstOriginHost[2] }; // (a copy: the caller may pass the info of dst)
	const uint32_t nSrc = s.nVoxels;
	hipStream_t st = (hipStream_t)stream;
	if( ownerDrain( dst ) ) return 1; // steps already issued render the old scene
	SortedVoxels v;
	if( resampleList( who, s, xf->m, xf->t, (uint32_t)levelsOf( dstGridRes ), v, st ) ) return 1;
	REQUIRE( v.n >= 1, "%s: the transform would leave no voxel (no destination cell centre maps into one of the %u voxels)", who, nSrc );
	return adoptSortedOnGrid( dst, v, nSrc, origin, dstDps, dstGridRes, buildFlags, nOut, st ); // (the source is read before the old octree of dst goes)
}
// host only, no GPU call: the transform of two lattices in world space
MVRT_EXPORT int mvrt_cell_transform_from_world( const double world[12], const float srcLower[3], float srcDps, const float dstLower[3], float dstDps, mvrt_cell_transform* out )
{
	const char* who = "mvrt_cell_transform_from_world";
	REQUIRE( world && srcLower && dstLower && out, "%s: null argument", who );
	for( int k = 0; k < 12; k++ ) REQUIRE( world[k] - world[k] == 0.0, "%s: world[%d] is not finite", who, k );
	for( int k = 0; k < 3; k++ ) REQUIRE( srcLower[k] - srcLower[k] == 0.0f && dstLower[k] - dstLower[k] == 0.0f, "%s: a lower bound is not finite", who );
	REQUIRE( srcDps > 0.0f && srcDps - srcDps == 0.0f && dstDps > 0.0f && dstDps - dstDps == 0.0f, "%s: dps %g / %g is not finite and positive", who, (double)srcDps,
			 (double)dstDps );
	const double* w = world; // row i: w[4 i .. 4 i + 2] = W, w[4 i + 3] = the translation
	const double c00 = w[5] * w[10] - w[6] * w[9], c01 = w[6] * w[8] - w[4] * w[10], c02 = w[4] * w[9] - w[5] * w[8];
	const double det = w[0] * c00 + w[1] * c01 + w[2] * c02;
	REQUIRE( det != 0.0 && det - det == 0.0, "%s: the world matrix is singular (det = %g)", who, det );
	const double inv[9] = { c00 / det, ( w[2] * w[9] - w[1] * w[10] ) / det, ( w[1] * w[6] - w[2] * w[5] ) / det,
							c01 / det, ( w[0] * w[10] - w[2] * w[8] ) / det, ( w[2] * w[4] - w[0] * w[6] ) / det,
							c02 / det, ( w[1] * w[8] - w[0] * w[9] ) / det, ( w[0] * w[5] - w[1] * w[4] ) / det };
	for( int k = 0; k < 9; k++ ) REQUIRE( inv[k] - inv[k] == 0.0, "%s: the world matrix is singular (its inverse is not finite)", who );
	const double ratio = (double)dstDps / (double)srcDps, mOne = 16777216.0 /* 2^24 */, mMax = 1073741824.0 /* 2^30 */, tMax = 4503599627370496.0 /* 2^52 */;
	mvrt_cell_transform x;
	x.structBytes = (uint32_t)sizeof( x );
	x.reserved = 0;
	const double d[3] = { (double)dstLower[0] - w[3], (double)dstLower[1] - w[7], (double)dstLower[2] - w[11] };
	for( int i = 0; i < 3; i++ )
	{
		for( int j = 0; j < 3; j++ )
		{
			const double a = inv[3 * i + j] * ratio * mOne;
			REQUIRE( a >= -mMax && a <= mMax, "%s: m[%d] = %g * 2^24 is out of range (|m[k]| <= 2^30)", who, 3 * i + j, inv[3 * i + j] * ratio );
			x.m[3 * i + j] = llrint( a );
		}
		const double b = ( ( inv[3 * i] * d[0] + inv[3 * i + 1] * d[1] + inv[3 * i + 2] * d[2] ) - (double)srcLower[i] ) / (double)srcDps;
		const double tb = b * ( 2.0 * mOne );
		REQUIRE( tb >= -tMax && tb <= tMax, "%s: t[%d] = %g * 2^25 is out of range (|t[i]| <= 2^52)", who, i, b );
		x.t[i] = llrint( tb );
	}
	*out = x;
	return 0;
}
MVRT_EXPORT int mvrt_test_resample_stats( uint64_t out[24] )
{
	const ResampleStats r = resampleLastStats();
	REQUIRE( out, "mvrt_test_resample_stats: null out" );
	out[0] = r.levels;
	for( int l = 1; l < 22; l++ ) out[l] = r.frontier[l];
	out[22] = out[23] = 0;
	return 0;
}
