/*
 * mvrt.h -- C-ABI of libmvrt_hip.so, the MI355X-native (gfx950) replacement for the
 * reference's GPU hot path: sparse-voxel-octree traversal, wavefront path tracing with
 * stable live-ray compaction, and the host objects that own it.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository root).  Plain pointers and sizes only: no C++ or torch types.
 *
 * Conventions
 *   - all functions return 0 on success, non-zero on failure; mvrt_last_error() gives text.
 *     (The reference returns void and __debugbreak()s / abort()s: hipUtil.hpp:18-22,
 *     IntersectorOctreeGPU.hpp:48-51.  The header-only C++ mirrors in include/mvrt/ (IntersectorOctreeGPU.hpp, PathTracer.hpp) keep the
 *     void signatures and abort() on a non-zero status.)
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); calls are asynchronous on
 *     it unless stated otherwise, exactly like the reference (PathTracer.hpp:150-169).  Streams created with hipStreamNonBlocking are supported: a
 *     call returns only after its own scratch is no longer in use, and its outputs are ordered on `stream` (tests/test_gpu_stream_order.py).
 *   - "host" / "dev" in a parameter name says where the pointer must live.
 *   - vectors are 3 packed floats; matrices are 16 floats, column-major (glm).
 *   - camera = the 15 floats of CameraPinhole {m_o, m_front, m_up, m_right, m_tanHthetaY,
 *     m_lensR, m_focus} (renderCommon.hpp:77-83).
 *   - OctreeNode = the reference's 68-byte AoS node (voxCommon.hpp:133-138); VoxelAttirb = 8 bytes
 *     {uchar4 color, uchar4 emission} (voxCommon.hpp:121-125).
 */
#ifndef MVRT_H
#define MVRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVRT_MAX_FLOAT 3.402823466e+38F /* "miss" marker for t, vectorMath.hpp:79 */

typedef struct mvrt_svo mvrt_svo; /* IntersectorOctreeGPU (IntersectorOctreeGPU.hpp:21-275) */
typedef struct mvrt_pt mvrt_pt;	  /* PathTracer (PathTracer.hpp:14-170) */

/* ---- runtime ------------------------------------------------------------------------------ */
const char* mvrt_last_error( void );
int mvrt_device_count( int* count );			/* replaces oroGetDeviceCount, voxPTGPU.cpp:16-39 */
int mvrt_set_device( int device );				/* replaces oroCtxCreate/SetCurrent */
int mvrt_device_name( char* buf, int bufLen );	/* voxPTGPU.cpp:215 device name print */
int mvrt_stream_create( void** stream );		/* oroStreamCreate, voxPTGPU.cpp:41 */
int mvrt_stream_destroy( void* stream );
int mvrt_stream_synchronize( void* stream );	/* oroStreamSynchronize, voxPTGPU.cpp:194 */
int mvrt_device_synchronize( void );
/* plain device buffers for callers without their own allocator (hipUtil.hpp:48-74 Buffer) */
int mvrt_malloc( void** dev, uint64_t bytes );
int mvrt_free( void* dev );
int mvrt_memcpy_h2d( void* dev, const void* host, uint64_t bytes, void* stream );
int mvrt_memcpy_d2h( void* host, const void* dev, uint64_t bytes, void* stream );
int mvrt_memcpy_d2d( void* dstDev, const void* srcDev, uint64_t bytes, void* stream ); /* asynchronous on stream */

/* ---- IntersectorOctreeGPU ------------------------------------------------------------------ */
typedef struct mvrt_svo_info
{
	uint32_t numberOfNodes;	 /* m_numberOfNodes  (IntersectorOctreeGPU.hpp:267) */
	uint32_t numberOfVoxels; /* m_numberOfVoxels (:268) */
	float lower[3];			 /* m_lower (:269) */
	float upper[3];			 /* m_upper (:270) */
	float dps;				 /* m_dps (:271) */
	float emissionScale;	 /* m_emissionScale = 7.5 (:273) */
	uint32_t hasEmission;	 /* m_hasEmission (:274) */
	uint32_t embeddedMask;	 /* 1: child pointers carry the child's mask in bits 24-31 (voxCommon.hpp:7-9) */
	uint32_t gridRes;
	uint32_t levels;		   /* log2(gridRes) = maximum traversal stack depth */
	uint64_t totalDumpedVoxels; /* entries before de-duplication: fragments of a triangle build, n of mvrt_svo_build_voxels; 0 after an upload or an edit */
	uint32_t flavour;			/* layout behind mvrt_svo_node_buffer_dev: MVRT_FLAVOUR_* */
	uint32_t reserved;
} mvrt_svo_info;
#define MVRT_FLAVOUR_EMBEDDED 0 /* 64-byte lines {children[8] with the child's mask in bits 24-31, nVoxelsPSum[8]} */
#define MVRT_FLAVOUR_PLAIN 1	/* 64-byte lines {children[8], the 8 child masks in 2 words, 6 unused words}; nVoxelsPSum in a separate array */
#define MVRT_FLAVOUR_TREE 2		/* 16-byte two-level bricks {u8 childMask[8]; u32 ownMask; u32 base} (four per 64-byte line) */

int mvrt_svo_create( mvrt_svo** out );
int mvrt_svo_destroy( mvrt_svo* svo ); /* IntersectorOctreeGPU::cleanUp, :26-38 */
/* What a failed call leaves behind.  A handle holds a whole octree, derived tables included, or NONE (numberOfNodes == 0 in mvrt_svo_get_info); never anything in
 * between.  Every entry point that reads an octree refuses an empty handle on the host with a "no octree" error, before any GPU work.
 *   - build, build_ex, build_synthetic, upload and mvrt_pt_update_scene release the old octree first, like the reference: once their arguments are accepted, a
 *     failure leaves the handle EMPTY.
 *   - build_voxels and edit_voxels build the new arrays next to the old octree and release it only then: a failure up to there (every rejected argument, coordinate
 *     or op among them) leaves the old octree exactly as it was, a failure after it (the derived tables) leaves the handle empty. */

/* IntersectorOctreeGPU::build (:40-241): voxelize triangles (six-separating), sort, de-duplicate with
 * integer-mean attributes, build the octree DAG bottom-up and embed child masks -- all on the GPU.
 * vertices/vcolors/vemissions: nVertices*3 host floats (nVertices = 3 * triangles); vcolors/vemissions may
 * be NULL (white / black, voxUtil.hpp:49-61).  gridRes must be a power of two (:48-51).  Blocks until done,
 * like the reference (5 host syncs, :92-211).  Node numbering is deterministic and equals
 * buildOctreeDAGReference's creation order (IntersectorOctree.hpp:11-123); root = last node (:250). */
int mvrt_svo_build( mvrt_svo* svo, const float* verticesHost, const float* vcolorsHost, const float* vemissionsHost, uint64_t nVertices, void* stream,
					const float origin[3], float dps, int gridRes );

/* Same with options.  MVRT_BUILD_NO_DAG: every sibling group becomes a node (the reference with ENABLE_GPU_DAG off,
 * voxKernel.cu:322-334; node numbering = deterministic group order).  MVRT_BUILD_NO_EMBEDDED_MASK: child pointers stay
 * plain indices and a node's mask is read from the node (voxCommon.hpp:353-356); chosen automatically when the octree has
 * >= 0xFFFFFF nodes, the limit of the embedded form (IntersectorOctreeGPU.hpp:231).  MVRT_BUILD_CONSERVATIVE: conservative
 * voxelization -- every voxel a triangle touches -- instead of the six-separating one (VTContext's sixSeparating == false,
 * voxelization.hpp:186-189,296-301; the reference's GPU build hard-codes six-separating, voxKernel.cu:68,109, its CPU demo has the
 * switch, voxRT.cpp:107,389). */
#define MVRT_BUILD_NO_DAG 1
#define MVRT_BUILD_NO_EMBEDDED_MASK 2
#define MVRT_BUILD_CONSERVATIVE 4
int mvrt_svo_build_ex( mvrt_svo* svo, const float* verticesHost, const float* vcolorsHost, const float* vemissionsHost, uint64_t nVertices, void* stream,
					   const float origin[3], float dps, int gridRes, int flags );
/* Seeded synthetic octree for HBM-bound stress runs (BASELINE.json configs[4]): nRandomVoxels uniformly random cells of the
 * gridRes^3 grid (duplicates merge), hash-derived colours, ~1/256 emissive; generated, sorted and built on the GPU.
 * voxel i: h = splitmix64(seed + i); x = h & (res-1), y = (h >> 21) & (res-1), z = (h >> 42) & (res-1); c = splitmix64(h):
 * colour = (c & 0xFFFFFF) | 0x404040, emission = colour if (c >> 56) == 0 else 0. */
int mvrt_svo_build_synthetic( mvrt_svo* svo, int gridRes, uint64_t nRandomVoxels, uint64_t seed, const float origin[3], float dps, int flags, void* stream );

/* Voxel lists (new; the reference only voxelizes triangles).  Device arrays in; the calls block like mvrt_svo_build.  A rejected list leaves the handle exactly as it
 * was: arguments are checked on the host before any GPU call, coordinates (and ops) on the device before anything is replaced -- the message names the LOWEST offending
 * entry.  (A failed allocation: see mvrt_svo_destroy above.)
 *
 * Build from a voxel list.  xyzDev: 3 x uint32 per voxel, each in [0, gridRes).  attribsDev: VoxelAttirb per entry {uchar4 color, uchar4 emission} (8 bytes), or NULL =
 * white, no emission (voxUtil.hpp's defaults).  Duplicate coordinates merge exactly like the reference's `unique` (integer mean of RGB per channel, alpha stored as 255,
 * hasEmission = any emission RGB != 0).  flags: MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK only.  gridRes: power of two in [2, 2^21].  1 <= n < 2^32 - 1. */
int mvrt_svo_build_voxels( mvrt_svo* svo, const uint32_t* xyzDev, const uint32_t* attribsDev, uint64_t n, const float origin[3], float dps, int gridRes, int flags,
						   void* stream );
#define MVRT_VOXEL_REMOVE 0
#define MVRT_VOXEL_SET 1
/* Apply a batch of edits to an octree this library built (build, build_ex, build_synthetic, build_voxels, or an earlier edit; not an upload).  opsDev: one byte per entry
 * (NULL = all SET).  SET inserts the voxel or replaces its attributes (no averaging; alpha stored as 255); REMOVE deletes it (absent voxel: no-op).  Entries naming the same
 * voxel: the LAST one in the batch wins.  Grid, origin, dps, build flags and emission scale are kept; the flavour is whatever a fresh build of the resulting voxel set picks.
 * A batch that only re-colours existing voxels keeps the nodes and writes the attributes in place; any insertion or removal rebuilds the levels.  Fails (handle
 * unchanged) on a coordinate outside the grid, an unknown op byte, or an edit that would remove every voxel.  Through mvrt_pt_intersector( pt ): the steps issued
 * before finish first and render the old scene; the frame buffer is not cleared.  An uploaded octree becomes editable after one mvrt_svo_rebuild. */
int mvrt_svo_edit_voxels( mvrt_svo* svo, const uint32_t* xyzDev, const uint32_t* attribsDev, const uint8_t* opsDev, uint64_t n, void* stream );
/* The current voxel set, sorted by Morton code (= vIndex order): coordinates (3 x uint32) and attributes (8 bytes) into caller device arrays of numberOfVoxels entries;
 * either may be NULL.  Octrees built by this library only; for an upload call mvrt_svo_rebuild first, or list its voxels with mvrt_svo_walk_voxels. */
int mvrt_svo_read_voxels( const mvrt_svo* svo, uint32_t* xyzDev, uint32_t* attribsDev, void* stream );

/* The exposed faces of the voxel set as a quad mesh: the reference voxelizer's "Save As Mesh" (voxMesh.cpp:111-219, voxelMeshWriter.hpp) on the GPU, from the
 * sorted Morton codes and the cell index a build leaves resident.  For an octree built by this library (build, build_ex, build_synthetic, build_voxels, or any
 * edit of one), of every flavour; an uploaded octree is refused like mvrt_svo_read_voxels ("keeps no Morton codes"), an empty handle with the "no octree" error,
 * both before any GPU work.  The handle is never modified.  The calls block like mvrt_svo_build (the counts come back to the host).  Any output pointer may be
 * NULL.  A capacity smaller than the count is an error: the counts are still returned and NOTHING is written to the caller's arrays; all outputs NULL is the
 * sizing call (capacities are then ignored).  A failed allocation of scratch returns an error, leaves the octree whole and leaks nothing.
 *   - Exposure mask: per voxel, in vIndex order (the Morton rank, as in read_voxels), one byte.  Bit b is set when the neighbouring grid cell in direction b holds
 *     no voxel.  Directions in the reference's emission order (voxMesh.cpp:172-200): 0 = -Y, 1 = +Y, 2 = -Z, 3 = +X, 4 = +Z, 5 = -X.  A neighbour outside
 *     [0, gridRes) is empty, in all six directions (the reference tests x == 0 and relies on the missing code for x + 1 == gridRes: the same below 2^21, and no
 *     21-bit wrap at 2^21).  Bits 6-7 are 0.  nFaces = the sum of the popcounts.
 *   - Face list: ascending vIndex, within a voxel ascending direction.  Per face faceVoxel (the vIndex: it indexes the attribute buffer, so colours need no
 *     output of their own), faceDir, and four corners in the reference's winding.
 *   - Corners 0..7 of the voxel at (x, y, z) lie at the offsets 0 (0,0,0) 1 (1,0,0) 2 (1,0,1) 3 (0,0,1) 4 (0,1,0) 5 (1,1,0) 6 (1,1,1) 7 (0,1,1); the faces are
 *     -Y = 3,2,1,0  +Y = 4,5,6,7  -Z = 0,1,5,4  +X = 1,2,6,5  +Z = 2,3,7,6  -X = 3,0,4,7.
 *   - Positions: a corner with integer grid coordinate c in [0, gridRes] on an axis lies at lower + (float)c * dps with the lower and dps of mvrt_svo_info: one fp32
 *     multiply and one fp32 add, each rounded, no FMA.  A DELIBERATE difference from the reference's (origin + x * dps) + dps, by an ulp in places: a corner
 *     shared by neighbouring voxels has ONE bit pattern, so the mesh is watertight and can be welded.
 *   - Welded mesh: a corner's key is (cz * (gridRes + 1) + cy) * (gridRes + 1) + cx (a uint64 up to gridRes 2^21); the vertices are the distinct keys of all face
 *     corners in ascending key order, indices[f][k] = the rank of the key of face f's corner k.  Refused on the host, naming the count, when 4 * nFaces >= 2^32.
 * An uploaded octree gets its surface after one mvrt_svo_rebuild. */
/* voxMesh.cpp:138-148 (the six neighbour tests).  masksDev: numberOfVoxels bytes, NULL = count only. */
int mvrt_svo_surface_masks( const mvrt_svo* svo, uint8_t* masksDev, uint64_t* nFacesOut, void* stream );
/* voxMesh.cpp:119-128,172-200 (one quad per exposed face, its corners not shared).  faceVoxelDev / faceDirDev: faceCapacity entries; positionsDev: 12 floats per face (4 corners x xyz). */
int mvrt_svo_surface_quads( const mvrt_svo* svo, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, uint64_t* nFacesOut,
							void* stream );
/* The same faces over SHARED vertices (the reference writes eight points per voxel, voxMesh.cpp:113-129,204-218; welding is new).  indicesDev: 4 per face; verticesDev: 3 floats per vertex, vertexCapacity vertices. */
int mvrt_svo_surface_mesh( const mvrt_svo* svo, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev,
						   float* verticesDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, void* stream );
/* The same surface with coplanar faces merged into rectangles (new; the reference has no counterpart).  The rules of the three calls above hold word for word:
 * the accepted handles and the two refusals before any GPU work (unknown flag bits are refused there too), a handle that is never modified, a blocking call, any
 * output NULL, all NULL = the sizing call, a capacity below the count = counts returned and NOTHING written, scratch that leaks nothing.  gridRes up to 2^21.
 *   - Faces: exactly those of mvrt_svo_surface_masks, directions d = 0..5 as there.  A face with normal axis a lies in plane p = the voxel's coordinate on a and has
 *     the in-plane coordinates (u, v) = the voxel's coordinates on the two other axes, the lower-numbered axis being u: x -> (y, z), y -> (x, z), z -> (x, y).
 *   - Two faces are mergeable when they have the same d and p and their voxels' attribute entries are equal in all 8 bytes (colour, emission, both alpha bytes);
 *     with MVRT_SURFACE_MERGE_ANY_ATTRIBUTE the attributes are not looked at.
 *   - Step 1, rows: within one (d, p, v) a run is a maximal sequence of faces at consecutive u, each mergeable with its predecessor: (d, p, v, u0, du).
 *   - Step 2, stacks: among the runs with the same (d, p, u0, du) and the same attribute (any attribute with the flag) a rectangle is a maximal sequence at
 *     consecutive v: (d, p, u0, v0, du, dv).
 *     Both steps take the maximal chains of a relation between neighbours, so the result is unique and independent of any processing order.  It is deliberately
 *     NOT a greedy merge: an L-shaped region gives two rectangles, a staircase one per row.
 *   - Order: ascending (d, p, u0, v0); the anchor face at (u0, v0) belongs to exactly one rectangle, so the order is total.
 *   - Per rectangle: rectVoxel = the vIndex of the anchor face's voxel (it indexes the attribute buffer like faceVoxel), rectDir = d, rectSize = 2 x uint32
 *     (du, dv), positions = 12 floats, the four corners.  Corner k has the integer grid coordinate: the anchor voxel's coordinate plus the corner offset of face d's
 *     corner k (the tables above), the offset scaled by du on the u axis, by dv on the v axis and by 1 on the normal axis; its position is lower + (float)c * dps
 *     as above -- for a 1 x 1 rectangle the bits and the winding of mvrt_svo_surface_quads.
 *   - With MVRT_SURFACE_MERGE_WELD the corners are welded exactly as in mvrt_svo_surface_mesh: the same key, vertices = the distinct keys ascending,
 *     indices[r][k] = the rank of the key of rectangle r's corner k.  A welded MERGED mesh has T-junctions: the edge of a rectangle can pass through a corner of
 *     its neighbour without having a vertex there.  Refused on the host, naming the count, when 4 * nRects >= 2^32.  Without the flag non-NULL indicesDev or
 *     verticesDev is refused on the host and *nVerticesOut is 0.
 *   - For every input the sum of du * dv equals the nFaces of mvrt_svo_surface_masks, and the rectangles cover exactly the faces of mvrt_svo_surface_quads, none twice.
 * rectVoxelDev / rectDirDev: rectCapacity entries; rectSizeDev: 2 per rectangle; positionsDev: 12 floats per rectangle; indicesDev: 4 per rectangle; verticesDev: 3
 * floats per vertex, vertexCapacity vertices. */
#define MVRT_SURFACE_MERGE_ANY_ATTRIBUTE 1u
#define MVRT_SURFACE_MERGE_WELD 2u
int mvrt_svo_surface_merged( const mvrt_svo* svo, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev, uint8_t* rectDirDev,
							 uint32_t* rectSizeDev, float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut, uint64_t* nRectsOut,
							 uint64_t* nVerticesOut, void* stream );

/* The enclosed empty cells of the voxel set, and the fill that makes a shell solid (new; the reference has none).  The work grows with the number of voxels, not
 * with the gridRes^3 cells of the grid.  Definitions:
 *   - Grid: [0, R)^3 with R = gridRes.  An empty cell is a grid cell without a voxel.
 *   - Neighbours: two empty cells are neighbours when they share a FACE (6-connectivity).  Diagonal contact does not connect.
 *   - Exterior: an empty cell is exterior when its connected component contains a cell with a coordinate equal to 0 or R - 1 -- the rule of
 *     mvrt_svo_surface_masks: outside the grid is empty.
 *   - Enclosed: every other empty cell.  Its component is a region.
 *   - Listing order: the enclosed cells in ascending Morton code (the order of mvrt_svo_read_voxels, x in bit 0 of each group); regions are numbered 0, 1, ... in
 *     order of first appearance in that list, so region[0] == 0 and a new id is always the previous maximum + 1.
 *   - The result is a property of the voxel set alone: unique and independent of any processing order.
 * mvrt_svo_enclosed_cells follows the rules of mvrt_svo_surface_quads word for word: every octree this library built or edited is accepted, in every flavour, the
 * tree flavour included (only the codes are read); an upload is refused ("keeps no Morton codes": it works after one mvrt_svo_rebuild), an empty handle too ("no
 * octree"), both before any GPU work.  The handle is never modified.  The call blocks (the counts come back to the host).  xyzDev: 3 x uint32 per cell, regionDev:
 * one uint32 per cell, `capacity` cells each; any output may be NULL, all arrays NULL is the sizing call (capacity is then ignored).  A capacity below the count is
 * an error: the counts are still returned and NOTHING is written.  A listing of 2^32 cells or more is refused on the host, the message names the count and the
 * counts are still returned.  Zero enclosed cells is a success with both counts 0.  gridRes up to 2^21.  A failed allocation of scratch returns an error, leaves
 * the octree whole and leaks nothing. */
int mvrt_svo_enclosed_cells( const mvrt_svo* svo, uint64_t capacity, uint32_t* xyzDev /* 3 per cell */, uint32_t* regionDev, uint64_t* nCellsOut, uint64_t* nRegionsOut,
							 void* stream );
/* Fill the enclosed cells: the handle's octree becomes exactly what mvrt_svo_edit_voxels leaves when given the cells of mvrt_svo_enclosed_cells, each with
 * fillAttribHost (8 bytes, VoxelAttirb {color, emission}; NULL = white, no emission) and MVRT_VOXEL_SET -- nodes and numbering, attributes with alpha stored as
 * 255, the recomputed hasEmission, the flavour a fresh build picks, the resident derived tables, the kept build flags, origin, dps and emission scale.  Existing
 * voxels keep their attributes.  The cells never travel to the host.  Failures and ordering are the edit's: the new arrays are built next to the old octree, a
 * failure before they are adopted leaves the handle unchanged, one after that leaves it empty (see mvrt_svo_destroy above); through mvrt_pt_intersector( pt ) the
 * steps issued before finish first and the frame buffer is not cleared; every mvrt_device_octree view of the handle is invalidated.  With zero enclosed cells the
 * call succeeds with *nFilledOut = 0 and leaves the handle untouched (no rebuild, views stay valid).  Refused with the handle unchanged: an upload, an empty
 * handle, and numberOfVoxels + nCells >= 2^32 - 1 (the message names the count).  nFilledOut may be NULL. */
int mvrt_svo_fill_enclosed( mvrt_svo* svo, const uint8_t fillAttribHost[8] /* VoxelAttirb, NULL = white, no emission */, uint64_t* nFilledOut, void* stream );
/* The enclosed cells with their nearest voxel, and the fill that takes its colours from it (new; the reference has none).  With A = the voxel set and c an
 * enclosed cell:
 *   - d2(c) = min over v in A of |c - v|^2 and near(c) = the lowest vIndex among the voxels that attain the minimum, as defined for mvrt_svo_distance_cells below.
 *     The minimum is over ALL of A: there is no radius.
 *   - dist2 < 2^20 always: no voxel lies in the open ball of radius sqrt( d2 ) around c, and every cell of that ball is an enclosed cell of c's region.  A
 *     listing holds fewer than 2^32 cells, so ( 4 / 3 ) pi d2^( 3 / 2 ) < 2^32.
 * mvrt_svo_enclosed_nearest: cells, order, xyzDev and regionDev are exactly what mvrt_svo_enclosed_cells writes (ascending Morton code), so the arrays of the two
 * calls align.  dist2Dev = d2(c), nearestDev = near(c) as a vIndex, attribsDev = colour RGB and emission RGB of voxel near(c) with both alpha bytes 255 (8 bytes
 * per cell; the rule of MVRT_VOXEL_SET and of the ball dilation).  Together they are the exact interior distance field of a closed shape: the depth of every
 * inside cell, and the largest inscribed ball of a cavity.  The call follows the rules of mvrt_svo_enclosed_cells word for word: every octree this library built or
 * edited is accepted, in every flavour (only the codes and the attributes are read); an upload is refused ("keeps no Morton codes"), an empty handle too ("no
 * octree"), both before any GPU work.  The handle is never modified.  The call blocks.  `capacity` cells per array; any output may be NULL, all five arrays NULL is
 * the sizing call (capacity is then ignored), which costs what the sizing call of mvrt_svo_enclosed_cells costs: the distances are not computed.  A capacity
 * below the count is an error: the counts are still returned and NOTHING is written.  A listing of 2^32 cells or more is refused on the host, the message names the
 * count and the counts are still returned.  Zero enclosed cells is a success with both counts 0.  A failed allocation of scratch returns an error, leaves the
 * octree whole, leaks nothing and has written nothing. */
int mvrt_svo_enclosed_nearest( const mvrt_svo* svo, uint64_t capacity, uint32_t* xyzDev /* 3 per cell */, uint32_t* regionDev, uint32_t* dist2Dev,
							   uint32_t* nearestDev /* vIndex */, uint32_t* attribsDev /* 8 bytes per cell */, uint64_t* nCellsOut, uint64_t* nRegionsOut, void* stream );
/* Fill the enclosed cells with the colours of the shell: the handle's octree becomes exactly what mvrt_svo_edit_voxels leaves when given the cells of
 * mvrt_svo_enclosed_nearest with the attributes it lists and MVRT_VOXEL_SET.  near(c) is taken on the set BEFORE the fill.  A shell with emission makes emissive
 * inside cells: hasEmission is recomputed over all voxels, and a cell behind an emissive voxel carries that voxel's emission bytes.  Everything else follows
 * mvrt_svo_fill_enclosed word for word: the cells never travel to the host; failures and ordering are the edit's (a failure before the new arrays are adopted
 * leaves the handle unchanged, one after that leaves it empty; steps issued before finish first; every mvrt_device_octree view is invalidated); with zero enclosed
 * cells the call succeeds with *nFilledOut = 0 and leaves the handle untouched (no rebuild, views stay valid).  Refused with the handle unchanged: an upload, an
 * empty handle, and numberOfVoxels + nCells >= 2^32 - 1 (the message names the count).  nFilledOut may be NULL.  mvrt_svo_fill_enclosed itself is unchanged. */
int mvrt_svo_fill_enclosed_nearest( mvrt_svo* svo, uint64_t* nFilledOut, void* stream );

/* A coarser level of detail of the voxel set, made from the voxels themselves (new; the reference voxelizes the triangles again at every resolution, and a set
 * built from a voxel list, an edit, a fill or an upload has no triangles).  Definitions, with R = gridRes of the source, L = log2 R, k = levelsDown in
 * [1, L - 1], so that the coarse grid has R' = R >> k >= 2:
 *   - The coarse cell of a voxel (x, y, z) is (x >> k, y >> k, z >> k); its Morton code is the voxel's code >> 3k.
 *   - count(c): the number of source voxels in cell c, 1 .. 8^k.
 *   - Cell c is KEPT when count(c) >= minCount, a uint64 in [1, 8^k].  minCount = 1 keeps every occupied cell: a conservative superset of the fine set.  A larger
 *     value drops thin features: a single stray fine voxel no longer becomes a whole coarse voxel.
 *   - Attribute of a kept cell, per channel R, G, B of colour and of emission: floor( sum of the channel / count ) with an EXACT integer sum (64-bit: a cell may
 *     hold 2^32 - 2 voxels, 255 times that needs 40 bits).  Both alpha bytes are stored as 255; the alpha bytes of the source are not read.  This is the
 *     reference's unique rule (voxKernel.cu:201-210): with minCount = 1 the result is what mvrt_svo_build_voxels makes of the shifted list wherever that call's
 *     32-bit sums do not overflow (a cell of more than 2^31 / 255 voxels).
 *   - Order: ascending coarse Morton code, the vIndex order of the coarse octree.
 *   - The result is a property of the voxel set alone: integer sums make it independent of any processing order.
 * mvrt_svo_coarse_voxels, the listing, follows the rules of mvrt_svo_enclosed_cells word for word: every octree this library built or edited is accepted, in every
 * flavour, the tree flavour included (only the codes and the attributes are read); an upload is refused ("keeps no Morton codes": it works after one
 * mvrt_svo_rebuild), an empty handle too ("no octree"); levelsDown outside [1, L - 1] is refused (the message names the range), minCount outside [1, 8^k] too; all
 * refusals happen on the host before any GPU work.  The handle is never modified.  The call blocks.  Per kept cell, into caller device arrays of `capacity`
 * cells: xyzDev 3 x uint32 coarse coordinates, attribsDev 8 bytes, countDev one uint32 = count(c).  Any output may be NULL; all NULL is the sizing call (capacity is
 * then ignored).  A capacity below the count is an error: the count is still returned and NOTHING is written.  Zero kept cells is a success with *nOut = 0.  A failed
 * allocation of scratch returns an error, leaves the octree whole and leaks nothing.  gridRes up to 2^21: the shift reaches 60 bits. */
int mvrt_svo_coarse_voxels( const mvrt_svo* svo, int levelsDown, uint64_t minCount, uint64_t capacity, uint32_t* xyzDev /* 3 per cell, coarse coordinates */,
							uint32_t* attribsDev /* 8 bytes per cell */, uint32_t* countDev /* fine voxels per cell */, uint64_t* nOut, void* stream );
/* dst becomes exactly the octree mvrt_svo_build_voxels would build from that listing at gridRes >> levelsDown with buildFlags (MVRT_BUILD_NO_DAG |
 * MVRT_BUILD_NO_EMBEDDED_MASK only; any other bit is refused): same nodes, numbering, flavour choice, cell index and prefix tables, vIndex = Morton rank.  The list
 * never travels to the host and is neither encoded nor sorted again.  lower = the source's; dps' = dps * 2^k, one fp32 multiply by an exact power of two (a
 * non-finite product is refused); gridRes = R'; upper = lower + dps' * R' is therefore bit-identical to the source's.  hasEmission is recomputed from the kept
 * cells, totalDumpedVoxels = the source's numberOfVoxels, the emission scale is the destination handle's own and is not touched.  dst == src is allowed: the
 * in-place LOD.  Otherwise src is never modified.  Refusals are the listing's, on the host; zero kept cells is refused with dst unchanged ("would leave no
 * voxel").  Failures are the voxel-list build's: the new arrays are built next to whatever dst holds, every failure before they are adopted leaves dst exactly as
 * it was, one after that leaves dst empty (see mvrt_svo_destroy above); src != dst stays whole throughout.  Through mvrt_pt_intersector( pt ) as dst: the steps
 * issued before finish first and render the old scene, the frame buffer is not cleared; every mvrt_device_octree view of dst is invalidated.  Blocks like
 * mvrt_svo_build. */
int mvrt_svo_coarsen( const mvrt_svo* src, mvrt_svo* dst, int levelsDown, uint64_t minCount, int buildFlags, void* stream );

/* Dilation, erosion, closing and opening of the voxel set (new; the reference has none).  Definitions, on the grid [0, R)^3 with R = gridRes and A = the voxel
 * set of the handle:
 *   - Structuring element e: MVRT_MORPH_FACES = the 6 face neighbours, MVRT_MORPH_CUBE = the 26 neighbours of the 3x3x3 block.  N_e(c) = the e-neighbours of
 *     cell c that lie INSIDE the grid.
 *   - One dilation step: D(A) = A + { c in the grid, c not in A, N_e(c) meets A }.  It is clipped to the grid: a neighbour coordinate of -1 or R does not exist,
 *     and at R = 2^21 nothing wraps in the 21 bits per axis of a code.  A new cell c takes, per channel R, G, B of colour and of emission,
 *     floor( sum over the voxels of N_e(c) in A / their number ), the number being 1..6 or 1..26; both alpha bytes are stored as 255, the alpha bytes of the source
 *     are not read.  This is the reference's unique rule (voxKernel.cu:201-210) and that of mvrt_svo_coarse_voxels; integer sums make it independent of any
 *     processing order.  Voxels of A keep all 8 attribute bytes verbatim.
 *   - One erosion step: E(A) = { v in A : N_e(v) lies in A }.  Cells outside the grid count as OCCUPIED here -- on purpose the opposite of
 *     mvrt_svo_surface_masks, where outside is empty: a build puts the extreme voxels of every model on the grid border, and with outside = empty every closing
 *     would eat exactly those.  With this rule D and E are adjoint on the subsets of the grid: E(A) = grid \ D(grid \ A), a closing contains A, an opening lies in
 *     A, and both are idempotent, for every A, e and number of steps.  Surviving voxels keep all 8 bytes verbatim.
 *   - k steps = the single step applied k times; the attributes of step i come from the set after step i - 1, so colour spreads outward layer by layer.
 *     steps in [1, 64].
 *   - Closing: k dilation steps, then k erosion steps.  Cells of A keep their bytes, an added cell carries the attribute its dilation step gave it.
 *   - Opening: the SET D^k(E^k(A)), a subset of A; every voxel of it keeps its ORIGINAL 8 bytes.  An opening is a pure removal, the same as mvrt_svo_edit_voxels
 *     with MVRT_VOXEL_REMOVE on A \ opening; the means of its dilation half are not used.
 *   - Every result is a property of the voxel set alone.
 * The listings give one step and follow the rules of mvrt_svo_enclosed_cells word for word: every octree this library built or edited is accepted, in every
 * flavour, the tree flavour included (only the codes and the attributes are read); an upload is refused ("keeps no Morton codes": it works after one
 * mvrt_svo_rebuild), an empty handle too ("no octree"), an unknown element too; all refusals happen on the host before any GPU work.  The handle is never
 * modified.  The calls block.  Arrays hold `capacity` entries; any output may be NULL, all NULL is the sizing call (capacity is then ignored).  A capacity below the
 * count is an error: the count is still returned and NOTHING is written.  Zero entries is a success.  A failed allocation of scratch returns an error, leaves the
 * octree whole and leaks nothing.  One step whose (voxel, empty neighbour) pairs number 2^32 - 1 or more is refused.
 * mvrt_svo_dilation_cells: the cells D(A) \ A in ascending Morton code: xyzDev 3 x uint32, attribsDev 8 bytes, countDev one uint32 = the occupied neighbours the
 * mean was taken over.  mvrt_svo_erosion_voxels: the voxels A \ E(A), the ones a step removes, as ascending vIndex. */
#define MVRT_MORPH_FACES 0
#define MVRT_MORPH_CUBE 1
int mvrt_svo_dilation_cells( const mvrt_svo* svo, int element, uint64_t capacity, uint32_t* xyzDev /* 3 per cell */, uint32_t* attribsDev /* 8 bytes per cell */,
							 uint32_t* countDev /* occupied neighbours, 1..26 */, uint64_t* nOut, void* stream );
int mvrt_svo_erosion_voxels( const mvrt_svo* svo, int element, uint64_t capacity, uint32_t* vIndexDev, uint64_t* nOut, void* stream );
/* In place: the handle's octree becomes exactly what mvrt_svo_edit_voxels leaves when given the net added cells with their attributes (MVRT_VOXEL_SET) and the net
 * removed voxels (MVRT_VOXEL_REMOVE) -- nodes and numbering, alpha 255 on new cells, the recomputed hasEmission, the flavour a fresh build picks, the derived
 * tables, the kept build flags, origin, dps and emission scale.  The steps run on sorted lists of codes and attributes; the levels are built ONCE per call, whatever
 * `steps` is.  Failures and ordering are the edit's: the new arrays are built next to the old octree, a failure before they are adopted leaves the handle
 * unchanged, one after that leaves it empty (see mvrt_svo_destroy above); through mvrt_pt_intersector( pt ) the steps issued before finish first and the frame
 * buffer is not cleared; every mvrt_device_octree view of the handle is invalidated.  A call that changes nothing (a dilation or an erosion of a full grid, a
 * closing that adds nothing) succeeds with 0 and leaves the handle untouched, its views valid.  Refused with the handle unchanged: an upload, an empty handle, an
 * unknown element, steps outside [1, 64], a voxel count that would reach 2^32 - 1 at any step (the message names the step and the count), and an erosion or
 * opening that would leave no voxel.  The count pointer may be NULL: the cells added by a dilation, the voxels removed by an erosion, the NET cells a closing adds
 * and the NET voxels an opening removes. */
int mvrt_svo_dilate( mvrt_svo* svo, int element, int steps, uint64_t* nAddedOut, void* stream );
int mvrt_svo_erode( mvrt_svo* svo, int element, int steps, uint64_t* nRemovedOut, void* stream );
int mvrt_svo_close( mvrt_svo* svo, int element, int steps, uint64_t* nAddedOut, void* stream );
int mvrt_svo_open( mvrt_svo* svo, int element, int steps, uint64_t* nRemovedOut, void* stream );

/* Round offsets: the exact distance band and dilation, erosion, closing and opening with a ball (new; the reference has none).  Definitions, on the grid [0, R)^3
 * with R = gridRes and A = the voxel set of the handle; radius2 = rho is a uint32 in [1, 1024], so the reach k = floor( sqrt( rho ) ) is at most 32:
 *   - Ball: B(rho) = { o in Z^3 : ox^2 + oy^2 + oz^2 <= rho }.  rho = 1 is the FACES element plus the centre, rho = 3 the CUBE element plus the centre, rho = 2 the
 *     18-neighbourhood.
 *   - Outer distance: for an in-grid cell c not in A, d2(c) = min over v in A of |c - v|^2, the exact integer squared distance; near(c) = the lowest vIndex among
 *     the voxels that attain the minimum.
 *   - Ball dilation: D_rho(A) = A + { c in the grid, c not in A, d2(c) <= rho }.  It is clipped to the grid: nothing wraps at coordinate 0, at R - 1, or in the 21
 *     bits per axis of a code at R = 2^21.  A new cell takes colour RGB and emission RGB of voxel near(c), with both alpha bytes stored as 255 (the rule of
 *     MVRT_VOXEL_SET).  This is not a mean: a round offset keeps colours crisp, and the tie rule makes it unique.  Voxels of A keep all 8 bytes verbatim.
 *   - Depth: for v in A, e2(v) = min over IN-GRID cells c not in A of |v - c|^2.  Cells outside the grid count as occupied, the rule of mvrt_svo_erode, for the
 *     reason given there.  If the grid is full, e2 is infinite.
 *   - Ball erosion: E_rho(A) = { v in A : e2(v) > rho }.  With this rule E_rho(A) = grid \ D_rho(grid \ A), the closing C_rho = E_rho(D_rho(A)) contains A, the
 *     opening O_rho = D_rho(E_rho(A)) lies in A, and both are idempotent, for every A and rho.
 *   - Closing: cells of A keep their bytes, an added cell carries the attribute the dilation gave it.
 *   - Opening: a pure removal: every surviving voxel keeps its ORIGINAL 8 bytes.
 *   - A ball of rho is one operation, not k repeated steps.  As sets, D_1 / E_1 equal one FACES step of mvrt_svo_dilate / _erode and D_3 / E_3 one CUBE step; the
 *     attributes of new cells differ: the nearest voxel here, the mean there.
 *   - Order: ascending Morton code.  Everything is integers, a property of the voxel set alone and independent of any schedule.
 * The listings follow the rules of mvrt_svo_dilation_cells / mvrt_svo_erosion_voxels word for word: every octree this library built or edited is accepted, in every
 * flavour; an upload is refused ("keeps no Morton codes"), an empty handle too ("no octree"), and a radius2 outside [1, 1024] (the message names the range); all
 * refusals happen on the host before any GPU work.  The handle is never modified.  The calls block.  Any output may be NULL, all arrays NULL is the sizing call
 * (capacity is then ignored).  A capacity below the count is an error: the count is still returned and NOTHING is written.  Zero entries is a success.  A failed
 * allocation of scratch returns an error, leaks nothing and has written nothing.  A pass whose records number 2^32 - 1 or more is refused; the message names the
 * pass and the count.
 * mvrt_svo_distance_cells: the cells of D_rho(A) \ A in ascending Morton code: xyzDev 3 x uint32, dist2Dev = d2, nearestDev = near as a vIndex, attribsDev the 8
 * bytes the cell would get.  mvrt_svo_depth_voxels: the voxels with e2 <= rho, that is A \ E_rho(A), as ascending vIndex with e2 in depth2Dev; with rho = 1024 it
 * doubles as a wall-thickness probe. */
int mvrt_svo_distance_cells( const mvrt_svo* svo, uint32_t radius2, uint64_t capacity, uint32_t* xyzDev /* 3 per cell */, uint32_t* dist2Dev,
							 uint32_t* nearestDev /* vIndex */, uint32_t* attribsDev /* 8 bytes per cell */, uint64_t* nOut, void* stream );
int mvrt_svo_depth_voxels( const mvrt_svo* svo, uint32_t radius2, uint64_t capacity, uint32_t* vIndexDev, uint32_t* depth2Dev, uint64_t* nOut, void* stream );
/* In place, following mvrt_svo_dilate .. _open word for word: the handle's octree becomes exactly what mvrt_svo_edit_voxels leaves when given the net added cells
 * with their attributes (MVRT_VOXEL_SET) and the net removed voxels (MVRT_VOXEL_REMOVE); the halves run on sorted lists and the levels are built ONCE per call.
 * Failures and ordering are the edit's.  A call that changes nothing succeeds with 0 and leaves the handle untouched, its views valid.  Refused with the handle
 * unchanged: an upload, an empty handle, a radius2 outside [1, 1024], a voxel count that would reach 2^32 - 1, and an erosion or opening that would leave no
 * voxel.  The count pointer may be NULL: the cells added by a dilation, the voxels removed by an erosion, the NET cells a closing adds and the NET voxels an
 * opening removes. */
int mvrt_svo_dilate_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nAddedOut, void* stream );
int mvrt_svo_erode_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nRemovedOut, void* stream );
int mvrt_svo_close_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nAddedOut, void* stream );
int mvrt_svo_open_ball( mvrt_svo* svo, uint32_t radius2, uint64_t* nRemovedOut, void* stream );

/* Connected components of the voxel set (new; the reference has none).  Definitions, on the grid [0, R)^3 with R = gridRes and A = the voxel set of the handle:
 *   - Connectivity e: MVRT_MORPH_FACES (6) or MVRT_MORPH_CUBE (26), the structuring elements above.
 *   - Two voxels are adjacent when one is an e-neighbour of the other INSIDE the grid: nothing wraps at coordinate 0, at R - 1, or in the 21 bits per axis of a code
 *     at R = 2^21.  A component is a class of the transitive closure of adjacency.
 *   - Labels: the components are numbered 0, 1, ... in order of first appearance in vIndex order (ascending Morton code): label[0] == 0, and a new label is always
 *     the previous maximum + 1 -- the numbering rule of mvrt_svo_enclosed_cells.
 *   - Per component: size = its voxels (uint32); first = its lowest vIndex (uint32); box = 6 x uint32: min x, y, z, then max x, y, z, inclusive.
 *   - Everything is a property of the voxel set alone: integers only, independent of any schedule.
 * mvrt_svo_components, the listing, follows the rules of mvrt_svo_enclosed_cells / mvrt_svo_dilation_cells word for word: every octree this library built or
 * edited is accepted, in every flavour, the tree flavour included (only the codes are read); an upload is refused ("keeps no Morton codes": it works after one
 * mvrt_svo_rebuild), an empty handle too ("no octree"), an unknown element too; all refusals happen on the host before any GPU work.  The handle is never
 * modified.  The call blocks.  labelDev holds numberOfVoxels entries in vIndex order; sizeDev, firstDev and boxDev hold componentCapacity components.  Any output
 * may be NULL; all four arrays NULL is the sizing call (componentCapacity is then ignored, as it is when labelDev is the only array).  A componentCapacity below the
 * count with a per-component array given is an error: the counts are still returned and NOTHING is written, labelDev included.  *nComponentsOut = the number of
 * components, *largestOut = the size of the largest.  A failed allocation of scratch returns an error, leaves the octree whole, leaks nothing and has written
 * nothing. */
int mvrt_svo_components( const mvrt_svo* svo, int element, uint32_t* labelDev /* numberOfVoxels, vIndex order */, uint64_t componentCapacity, uint32_t* sizeDev,
						 uint32_t* firstDev, uint32_t* boxDev /* 6 per component */, uint64_t* nComponentsOut, uint64_t* largestOut, void* stream );
/* In place: component c is kept when size(c) >= minVoxels and ( keepLargest == 0 or rank(c) < keepLargest ), rank ordering the components by (size descending,
 * label ascending): a tie in size goes to the component that appears first.  minVoxels >= 1; minVoxels == 1 && keepLargest == 0 keeps everything.  The handle
 * becomes exactly what mvrt_svo_edit_voxels leaves when given the voxels of the dropped components with MVRT_VOXEL_REMOVE -- nodes and numbering, the surviving
 * attributes (all 8 bytes verbatim), the recomputed hasEmission, the flavour a fresh build picks, the derived tables, the kept build flags, origin, dps and
 * emission scale, totalDumpedVoxels 0.  The list is compacted on the device and the levels are built once.  Failures and ordering are the edit's: the new arrays
 * are built next to the old octree, a failure before they are adopted leaves the handle unchanged, one after that leaves it empty (see mvrt_svo_destroy above);
 * through mvrt_pt_intersector( pt ) the steps issued before finish first and the frame buffer is not cleared; every mvrt_device_octree view of the handle is
 * invalidated.  A call that drops nothing succeeds, reports 0 removed and leaves the handle untouched, its views valid.  Refused with the handle unchanged: an
 * upload, an empty handle, an unknown element, minVoxels == 0, and a selection that would leave no voxel ("would leave no voxel").  *nRemovedOut = the voxels
 * removed, *nKeptOut = the components kept; either may be NULL. */
int mvrt_svo_keep_components( mvrt_svo* svo, int element, uint64_t minVoxels, uint32_t keepLargest, uint64_t* nRemovedOut, uint64_t* nKeptOut, void* stream );

/* Boolean operations between two voxel sets, the second moved by an integer cell offset (new; the reference has none).  Definitions:
 *   - Sets: on the grid [0, R)^3 with R = gridRes of handle a, A = the voxel set of a and B = the voxel set of b, taken cell for cell: b's lower and dps are not
 *     read, and b's gridRes need not equal a's.
 *   - Offset o: three int32, each in [-2^21, 2^21]; NULL = zero.  B' = { v + o : v in B, v + o in [0, R)^3 }.  The sum is taken in an integer type that cannot
 *     wrap: a translated coordinate of -1 or R does not exist, R = 2^21 included, and nothing is folded back into the 21 bits per axis of a code.
 *     nClipped = |B| - |B'|.  Translation is injective, so B' has no duplicates.
 *   - op: MVRT_COMBINE_UNION = A + B', MVRT_COMBINE_INTERSECTION = A n B', MVRT_COMBINE_DIFFERENCE = A \ B', MVRT_COMBINE_XOR = ( A \ B' ) + ( B' \ A ).
 *   - Attributes: a result voxel that is in A keeps a's 8 bytes verbatim.  A voxel of B' alone takes b's colour RGB and emission RGB with both alpha bytes stored
 *     as 255, the rule of MVRT_VOXEL_SET.  flags bit 0, MVRT_COMBINE_ATTRIB_B: the voxels of A n B' that survive (under UNION and INTERSECTION only) take b's
 *     attribute by that rule instead; it has no effect under DIFFERENCE and XOR.  Any other flags bit is refused.
 *   - Order: ascending Morton code in a's grid.  Everything is integers, a property of the two sets and the offset alone.
 * mvrt_svo_combine_voxels, the listing, follows the rules of mvrt_svo_dilation_cells word for word: every octree this library built or edited is accepted for
 * either handle, in every flavour, the tree flavour included (only the codes and the attributes are read); an upload is refused ("keeps no Morton codes": it
 * works after one mvrt_svo_rebuild), an empty handle too ("no octree"), an unknown op or flags bit too, and an offset component outside the range; all refusals
 * happen on the host before any GPU work.  Neither handle is modified.  The call blocks.  Arrays hold `capacity` entries: xyzDev 3 x uint32, attribsDev 8 bytes,
 * sourceDev one byte = 1 (in A only), 2 (in B' only) or 3 (in both).  Any output may be NULL, all three arrays NULL is the sizing call (capacity is then
 * ignored).  A capacity below the count is an error: the counts are still returned and NOTHING is written.  An empty result is a success with *nOut = 0.
 * *nOverlapOut = |A n B'| whatever the op, *nClippedOut = nClipped.  A failed allocation of scratch returns an error, leaves both octrees whole, leaks nothing
 * and has written nothing. */
#define MVRT_COMBINE_UNION 0
#define MVRT_COMBINE_INTERSECTION 1
#define MVRT_COMBINE_DIFFERENCE 2
#define MVRT_COMBINE_XOR 3
#define MVRT_COMBINE_ATTRIB_B 1u
int mvrt_svo_combine_voxels( const mvrt_svo* a, const mvrt_svo* b, int op, const int32_t offset[3], uint32_t flags, uint64_t capacity, uint32_t* xyzDev /* 3 per voxel */,
							 uint32_t* attribsDev /* 8 bytes per voxel */, uint8_t* sourceDev /* 1 = a only, 2 = b only, 3 = both */, uint64_t* nOut,
							 uint64_t* nOverlapOut /* |A n B'| */, uint64_t* nClippedOut, void* stream );
/* In place: a becomes exactly what mvrt_svo_edit_voxels leaves when given B' \ A with b's attributes as MVRT_VOXEL_SET (UNION and XOR), the overlap with b's
 * attributes as MVRT_VOXEL_SET (under MVRT_COMBINE_ATTRIB_B) and the voxels the operation drops as MVRT_VOXEL_REMOVE -- nodes and numbering, the recomputed
 * hasEmission, the flavour a fresh build picks, the derived tables, the kept build flags, origin, dps and emission scale, totalDumpedVoxels 0.  The lists never
 * travel to the host and the levels are built once.  Failures and ordering are the edit's: the new arrays are built next to the old octree, a failure before
 * they are adopted leaves a unchanged, one after that leaves it empty (see mvrt_svo_destroy above); b stays whole throughout.  Through mvrt_pt_intersector( pt )
 * as a the steps issued before finish first and the frame buffer is not cleared; every mvrt_device_octree view of a is invalidated.  a == b is allowed (b's list is
 * read before anything is replaced): with a non-zero offset the union is a directional smear.  A call that adds nothing, removes nothing and recolours nothing
 * succeeds, reports 0 / 0 and leaves the handle untouched, its views valid.  A call that only recolours under the flag behaves like the attribute-only edit: the
 * nodes are kept, the attributes are written in place and hasEmission is recomputed.  Refused with a unchanged: everything the listing refuses, a result of
 * 2^32 - 1 voxels or more (the message names the count) and an empty result ("would leave no voxel").  *nAddedOut = |B' \ A| where the op takes it, *nRemovedOut
 * = the voxels of A the op drops, *nClippedOut = nClipped; each may be NULL. */
int mvrt_svo_combine( mvrt_svo* a, const mvrt_svo* b, int op, const int32_t offset[3], uint32_t flags, uint64_t* nAddedOut, uint64_t* nRemovedOut, uint64_t* nClippedOut,
					  void* stream );

/* The voxel set of one octree resampled onto another grid under an affine map (new; the reference has none).  With mvrt_svo_combine behind it this is the rotated
 * or scaled stamp; mvrt_cell_transform_from_world below is the world-space alignment of two lattices.  Definitions, with S = the voxel set of src on [0, Rs)^3,
 * Rd = the destination gridRes, a power of two in [2, 2^21] as for mvrt_svo_build_voxels, and F = MVRT_TRANSFORM_FRAC_BITS = 24:
 *   - The rule.  For a destination cell c = (c0, c1, c2) in [0, Rd)^3:
 *       P_i = m[3i+0]*(2*c0+1) + m[3i+1]*(2*c1+1) + m[3i+2]*(2*c2+1) + t[i], taken in int64;
 *       s_i = floor( P_i / 2^(F+1) ), the floor towards minus infinity.
 *     Cell c belongs to the result when s lies in [0, Rs)^3 and is a voxel of S.  It then takes that voxel's colour RGB and emission RGB with both alpha bytes 255,
 *     the rule of MVRT_VOXEL_SET, and source(c) is that voxel's vIndex.
 *   - In words: m is the INVERSE map in Q24, destination cell space to source cell space, and t is its translation in Q25; the sample point is the centre of the
 *     destination cell.  The rule is nearest-neighbour resampling by inverse mapping: no holes under rotation, and no duplicates.
 *   - Limits: |m[k]| <= 2^30, so entries reach 64, and |t[i]| <= 2^52.  With 2*c+1 < 2^22 every |P_i| stays below 2^55: nothing can wrap.  The bounds are checked on
 *     the host; structBytes must be sizeof( mvrt_cell_transform ) and reserved must be 0.
 *   - Singular maps are legal: m need not be invertible, because only the inverse direction is ever evaluated.  An all-zero m sends every destination cell to the
 *     cell that t names.
 *   - Order: ascending Morton code in the destination grid.  Everything is integers: the result is a property of the set and the transform alone.
 *   - Two facts that pin the conventions.  A signed permutation about the grid centre with Rd == Rs gives a bijection, c_j -> c_j or Rs - 1 - c_j per axis, exact in
 *     Q24 (mirror of axis j: m = -2^24 on it, t = Rs * 2^25).  A = I/2 gives s = c >> 1, so each voxel becomes a 2x2x2 block; A = 2I gives s = 2c + 1: this is
 *     sub-sampling, NOT the count rule of mvrt_svo_coarsen.
 * mvrt_svo_resample_voxels, the listing, follows the rules of mvrt_svo_combine_voxels word for word: every octree this library built or edited is accepted, in every
 * flavour, the tree flavour included (only the codes and the attributes are read); an upload is refused ("keeps no Morton codes": it works after one
 * mvrt_svo_rebuild), an empty handle too ("no octree"); a bad transform or a bad gridRes is refused on the host, before any GPU work and
 * before the state of the handle is looked at (a null handle comes first of all).  src is never modified.  The
 * call blocks.  Arrays hold `capacity` entries: xyzDev 3 x uint32, attribsDev 8 bytes, sourceDev one uint32 = source(c).  Any output may be NULL, all three NULL is
 * the sizing call (capacity is then ignored).  A capacity below the count is an error: the count is still returned and NOTHING is written.  An empty result is a
 * success with *nOut = 0.  The destination grid is refined top-down, a frontier of nodes per level: a result, or an intermediate frontier, of 2^32 - 1 entries or
 * more is refused (the message names the count).  A failed allocation of scratch returns an error, leaks nothing and has written nothing. */
#define MVRT_TRANSFORM_FRAC_BITS 24
typedef struct mvrt_cell_transform
{
	uint32_t structBytes, reserved;
	int64_t m[9]; /* row-major, Q24 */
	int64_t t[3]; /* Q25 */
} mvrt_cell_transform;
int mvrt_svo_resample_voxels( const mvrt_svo* src, const mvrt_cell_transform* xf, int dstGridRes, uint64_t capacity, uint32_t* xyzDev /* 3 per voxel */,
							  uint32_t* attribsDev /* 8 bytes per voxel */, uint32_t* sourceDev /* vIndex in src */, uint64_t* nOut, void* stream );
/* Into a handle, by the rules of mvrt_svo_coarsen: dst becomes exactly the octree mvrt_svo_build_voxels would build from that listing with dstOriginHost, dstDps,
 * dstGridRes and buildFlags (MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK only; any other bit is refused): same nodes, numbering, flavour choice, cell index and
 * prefix tables, vIndex = Morton rank.  The list never travels to the host and is neither encoded nor sorted again.  hasEmission is recomputed from the result,
 * totalDumpedVoxels = the source's numberOfVoxels, the emission scale is the destination handle's own and is not touched.  dst == src is allowed: the list is
 * complete before anything is replaced.  Otherwise src is never modified.  Refusals are the listing's, on the host; an empty result is refused with dst unchanged
 * ("would leave no voxel").  Failures and ordering are the voxel-list build's: the new arrays are built next to whatever dst holds, every failure before they are
 * adopted leaves dst exactly as it was, one after that leaves dst empty (see mvrt_svo_destroy above); src != dst stays whole throughout.  Through
 * mvrt_pt_intersector( pt ) as dst: the steps issued before finish first and render the old scene, the frame buffer is not cleared; every mvrt_device_octree view
 * of dst is invalidated.  *nOut (may be NULL) = the voxels of the result.  Blocks like mvrt_svo_build. */
int mvrt_svo_resample( const mvrt_svo* src, mvrt_svo* dst, const mvrt_cell_transform* xf, const float dstOriginHost[3], float dstDps, int dstGridRes, int buildFlags,
					   uint64_t* nOut, void* stream );
/* Host only, no GPU call: the transform that aligns two lattices in world space.  world is 3x4 row-major, p_dst = W * p_src + w.  With Winv computed in double:
 * A = Winv * ( dstDps / srcDps ), b = ( Winv * ( dstLower - w ) - srcLower ) / srcDps, m[k] = llrint( A[k] * 2^24 ) and t[i] = llrint( b[i] * 2^25 ).  Refused: a
 * non-finite input, det W == 0 or a non-finite inverse ("singular"), a dps that is not finite and positive, and any entry outside the limits above. */
int mvrt_cell_transform_from_world( const double world[12], const float srcLower[3], float srcDps, const float dstLower[3], float dstDps, mvrt_cell_transform* out );

/* The nearest voxel of arbitrary lattice points, the distance from one voxel set to another, and the recolouring of one set from another (new; the reference has
 * none).  Definitions:
 *   - Set and queries: B = the voxel set of a handle.  A voxel is named by its vIndex, its Morton rank, the order of mvrt_svo_read_voxels.  A query is a point q
 *     of the integer cell lattice, three int32, each in [-2^22, 2^22]; it need not lie in the grid.
 *   - Distance and nearest voxel: d2(q) = min over v in B of |q - v|^2; near(q) = the lowest vIndex among the voxels that attain d2(q).  This is the rule of
 *     mvrt_svo_distance_cells and mvrt_svo_enclosed_nearest, without a radius and for any point.
 *   - Field widths: d2 is below 2^47 and is a uint64 everywhere in this interface; the packed 64-bit key of the distance band does not fit, ( d2, vIndex ) is
 *     compared as a pair.
 *   - Limit: maxDist2 is a uint64; UINT64_MAX means no limit, 0 is legal and is the membership test.  A query with d2(q) > maxDist2 reports dist2 = UINT64_MAX,
 *     nearest = 0xFFFFFFFF and all-zero attribute bytes.  Otherwise the answer is exact: the limit never changes an answer that lies within it.
 *   - Attributes: attribs(q) = colour RGB and emission RGB of voxel near(q) with both alpha bytes 255, the rule of MVRT_VOXEL_SET.
 *   - Determinism: everything is integers and a property of the set and the query alone, independent of any schedule.  A tie at equal d2 goes to the lower vIndex:
 *     a part of the set is passed over only when it lies STRICTLY further than the best distance so far.
 * The three calls follow mvrt_svo_combine_voxels word for word on refusals and on what a failure leaves: every octree this library built or edited is accepted, in
 * every flavour, the tree flavour included (only the codes and the attributes are read); an upload is refused ("keeps no Morton codes": it works after one
 * mvrt_svo_rebuild), an empty handle too ("no octree"), and a bad coordinate, offset or flags bit; all refusals happen on the host before any GPU work.  The calls
 * block.  A failed allocation of scratch returns an error, leaks nothing and has written nothing: nothing is written to a caller's array before the last
 * allocation and the capacity check have passed.
 * mvrt_svo_nearest_voxels: queryDev holds n x 3 int32 on the device, dist2Dev n uint64, nearestDev n uint32, attribsDev 8 bytes per query; any output may be NULL.
 * n == 0 is a success without a launch, n >= 2^32 is refused.  Answers come in the caller's order.  The handle is never modified.  The coordinates are on the
 * device and are not checked: one outside [-2^22, 2^22] gives an unspecified answer for that query alone (the arithmetic is 64-bit and cannot fault). */
int mvrt_svo_nearest_voxels( const mvrt_svo* svo, uint64_t n, const int32_t* queryDev /* 3 per query */, uint64_t maxDist2, uint64_t* dist2Dev, uint32_t* nearestDev,
							 uint32_t* attribsDev /* 8 bytes per query */, void* stream );
/* For every voxel v of a, in a's vIndex order, the query q = v - o in b's cell space; o is three int32 in [-2^21, 2^21], NULL = 0, as for mvrt_svo_combine_voxels.
 * Nothing is clipped: distances need no grid, and the gridRes of a and b need not be equal.  *nOut = a's voxel count; *maxDist2Out = the largest d2 within the
 * limit, the squared one-sided Hausdorff distance from A to B + o; *farthestOut = the lowest vIndex of a that attains it; *nZeroOut = the voxels of a with
 * d2 == 0, which equals nOverlap of mvrt_svo_combine_voxels on equal grids; *nBeyondOut = the voxels beyond the limit (with all of them beyond, *maxDist2Out is 0
 * and *farthestOut 0xFFFFFFFF).  Each may be NULL.  dist2Dev and nearestDev hold `capacity` entries; both NULL is the summary call (capacity is then ignored); a
 * capacity below the count with an array given is an error: *nOut is still returned and NOTHING is written.  a == b is allowed: with o = 0 every d2 is 0 and
 * nearest[i] = i.  The queries are made on the device from a's codes; nothing travels to the host but the five numbers.  Neither handle is modified. */
int mvrt_svo_nearest_between( const mvrt_svo* a, const mvrt_svo* b, const int32_t offset[3], uint64_t maxDist2, uint64_t capacity, uint64_t* dist2Dev, uint32_t* nearestDev,
							  uint64_t* nOut, uint64_t* maxDist2Out, uint32_t* farthestOut, uint64_t* nZeroOut, uint64_t* nBeyondOut, void* stream );
/* In place: dst becomes exactly what mvrt_svo_edit_voxels leaves when given every voxel v of dst that has a nearest voxel of src within the limit, as
 * MVRT_VOXEL_SET, with the word or words `flags` names (MVRT_TRANSFER_COLOUR = the colour word, MVRT_TRANSFER_EMISSION = the emission word; at least one, any
 * other bit is refused) of attribs( v - o ) taken in src, and the other word the voxel's own.  This is the attribute-only edit: nodes and numbering are kept, the
 * attributes are written in place, hasEmission is recomputed, totalDumpedVoxels ends 0, and through mvrt_pt_intersector( pt ) the steps issued before finish
 * first.  Voxels beyond the limit keep all 8 bytes verbatim.  near is taken in src BEFORE anything is written: dst == src is allowed, and with o = 0 it only
 * normalises the alpha bytes.  *nChangedOut = the voxels whose 8 bytes differ afterwards, *nBeyondOut = the voxels beyond the limit; either may be NULL.  A call
 * that changes no byte succeeds and leaves the handle untouched, its device views valid.  Failures are the edit's: a failed allocation leaves dst as it was. */
#define MVRT_TRANSFER_COLOUR 1u
#define MVRT_TRANSFER_EMISSION 2u
int mvrt_svo_transfer_attributes( mvrt_svo* dst, const mvrt_svo* src, const int32_t offset[3], uint64_t maxDist2, uint32_t flags, uint64_t* nChangedOut, uint64_t* nBeyondOut,
								  void* stream );

/* Exterior-only surface extraction without touching the octree, and the three extraction calls on face masks the caller supplies (new; the reference has
 * none).  Definitions:
 *   - Exterior mask of a voxel: one byte, directions d = 0..5 as in mvrt_svo_surface_masks (0 = -Y, 1 = +Y, 2 = -Z, 3 = +X, 4 = +Z, 5 = -X).  Bit d is set when the
 *     neighbour cell in direction d is outside the grid, or is empty and NOT an enclosed cell in the sense of mvrt_svo_enclosed_cells above (6-connectivity;
 *     exterior = the component holds a cell with a coordinate equal to 0 or gridRes - 1).  Bits 6-7 are 0.
 *   - (E1) It is the mask of mvrt_svo_surface_masks with the bits that look into an enclosed cell cleared.
 *   - (E2) It is the mask of mvrt_svo_surface_masks the same voxel has after mvrt_svo_fill_enclosed; a filled cell itself has no exposed face.
 *   - A shell nested inside another shell's cavity has no exterior face at all.  In a closed scene -- a room, a tunnel: everything inside the outer walls is
 *     enclosed -- only the outside of the block has exterior faces, exactly as the fill would make such a scene solid.
 *   - The result is a property of the voxel set alone: unique and independent of any processing order.
 * mvrt_svo_surface_exterior_masks follows the rules of mvrt_svo_surface_quads word for word: every octree this library built or edited is accepted, in every
 * flavour; an upload is refused ("keeps no Morton codes": it works after one mvrt_svo_rebuild), an empty handle too ("no octree"), both before any GPU work.  The
 * handle is never modified: no voxel is inserted, every vIndex stays.  The call blocks.  masksDev: numberOfVoxels bytes in vIndex order, NULL = counts only.
 * *nFacesOut = the sum of the popcounts of the exterior masks, *nHiddenOut = the faces of mvrt_svo_surface_masks minus those; either may be NULL.  Counts are
 * 64-bit.  gridRes up to 2^21.  A failed allocation of scratch returns an error, leaves the octree whole, leaks nothing and has written nothing to masksDev. */
int mvrt_svo_surface_exterior_masks( const mvrt_svo* svo, uint8_t* masksDev /* numberOfVoxels bytes in vIndex order, NULL = counts only */, uint64_t* nFacesOut,
									 uint64_t* nHiddenOut /* plain faces - exterior faces */, void* stream );
/* mvrt_svo_surface_quads / _mesh / _merged on a face set the caller supplies.  Each behaves exactly like its namesake -- handles, refusals, blocking, NULL
 * outputs, the sizing call, capacities, counts, order, corners, positions, the weld and the merge rule -- except that the faces are the set bits 0..5 of
 * masksDev: numberOfVoxels bytes in vIndex order, e.g. those of mvrt_svo_surface_exterior_masks, of mvrt_svo_surface_masks (the namesake's output, byte for
 * byte), or any selection of the caller's: one direction only, a clip region.
 *   - The masks are taken as given: a set bit whose neighbour cell is in fact occupied still yields its face.  Bits 6 and 7 are ignored.  masksDev is only read.
 *   - masksDev == NULL is refused on the host ("null masksDev"), like a null handle, before any GPU work.
 *   - All outputs NULL is the sizing call: *nFacesOut = the number of set bits 0..5 of the given masks.  All-zero masks are a success with 0 faces, nothing written.
 *   - mvrt_svo_surface_merged_masked takes the two flags of mvrt_svo_surface_merged; unknown bits are refused as there, and indicesDev / verticesDev need
 *     MVRT_SURFACE_MERGE_WELD as there.  The rectangles depend only on the given faces and their voxels' attributes.
 *   - Masks belong to the voxel set they were made for.  After mvrt_svo_edit_voxels, mvrt_svo_fill_enclosed or mvrt_svo_rebuild the vIndex order may have
 *     changed: stale masks are not detected, they are the caller's business.
 * mvrt_svo_surface_ao needs no counterpart: it takes a face list already, so the faces of a _masked call go straight in. */
int mvrt_svo_surface_quads_masked( const mvrt_svo* svo, const uint8_t* masksDev, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev,
								   uint64_t* nFacesOut, void* stream );
int mvrt_svo_surface_mesh_masked( const mvrt_svo* svo, const uint8_t* masksDev, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev,
								  uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, void* stream );
int mvrt_svo_surface_merged_masked( const mvrt_svo* svo, const uint8_t* masksDev, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev,
									uint8_t* rectDirDev, uint32_t* rectSizeDev, float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut,
									uint64_t* nRectsOut, uint64_t* nVerticesOut, void* stream );

/* The welded mesh smoothed by constrained surface nets (Gibson; new, the reference has none): the dual mesh of a binary voxel set has exactly the vertices and
 * quads of mvrt_svo_surface_mesh, only the vertex positions change.  Each vertex relaxes towards the mean of its edge neighbours and never leaves a box around
 * the lattice corner it came from.  Defined in integers, so the result is unique and independent of any schedule; one conversion to float at the end.
 *   - Mesh: the faces, their order, faceVoxel, faceDir, the welded vertices, their order (ascending corner key) and indices are exactly those of
 *     mvrt_svo_surface_mesh; with masksDev != NULL those of mvrt_svo_surface_mesh_masked for the same masks.  Only vertex positions differ.
 *   - Corner: vertex i has the integer lattice corner c_i in [0, gridRes]^3, decoded from its key.
 *   - Neighbours: N(i) = the vertices joined to i by an edge of at least one listed face: corners k and (k +- 1) mod 4 of the same quad.  Two such corners
 *     differ by +-1 on exactly one axis, so N(i) has at most 6 members, one per slot; the slots are the bits of the per-vertex neighbour mask: bit 0 = -x,
 *     1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z; bits 6-7 are 0.  n_i = |N(i)| >= 2.  u_ij = c_j - c_i, a signed unit vector.  The definition goes through the
 *     face list, not through occupancy: it holds for caller-supplied and exterior masks as well; a face listed from both sides adds nothing new.
 *   - Displacement: d_i = 3 x int32 in steps of 1 / MVRT_SMOOTH_STEPS_PER_CELL cell, 0 at the start.
 *   - Iteration k = 0, 1, ..., a Jacobi step (every vertex reads the d of iteration k - 1), per axis in exact integers:
 *       T_i = sum over j in N(i) of ( 256 u_ij + d_j ) - n_i d_i
 *       delta_i = rdiv( w_k T_i, 256 n_i ),  rdiv( a, b ) = sign( a ) * floor( ( 2|a| + b ) / ( 2 b ) ) for b > 0: nearest, ties away from zero, so that
 *       mirrored sets give mirrored meshes;  w_k = weightEven for even k, weightOdd for odd k
 *       d_i <- clamp( d_i + delta_i, -limit, +limit )
 *     Every axis of every vertex whose d_i + delta_i lay outside [-limit, limit] adds 1 to the call's clamped count, summed over all iterations.
 *     |w T| stays below 2^20.
 *   - Parameters: iterations 0..256 (default 4); weightEven, weightOdd -256..256 (256, 256: the plain Laplacian step; 128, -136 is Taubin's non-shrinking
 *     pair); limit 0..128 (127; 128 is half a cell); the reserved words must be 0.  A value outside its range and a non-zero reserved word are refused on
 *     the host, the message naming the field.  With limit <= 127 all vertices have distinct positions in fixed point: no two vertices meet, no quad
 *     collapses (at 128 the eight vertices of a lone voxel meet in its centre).
 *   - Position, per axis: q = 256 c + d (int32, at most 2^29 + 128); t = (float)q * 0.00390625f (the conversion rounds once, the scaling is exact);
 *     p = lower + t * dps, multiply and add each rounded to fp32, no FMA.  For d = 0, t == (float)c: iterations = 0 returns the bits of mvrt_svo_surface_mesh.
 * The rules of mvrt_svo_surface_mesh hold word for word: every octree this library built or edited is accepted, in every flavour; an upload ("keeps no Morton
 * codes") and an empty handle ("no octree") are refused before any GPU work; the handle is never modified; the call blocks; any output pointer may be NULL; all
 * arrays NULL is the sizing call, which runs no iteration (*clampedOut = 0); a capacity below the count is an error, the counts are still returned and NOTHING
 * is written; 4 * nFaces >= 2^32 is refused, naming the count; gridRes up to 2^21; a failed scratch allocation returns an error, leaves the octree whole and
 * leaks nothing.  displacementsDev and neighboursDev follow vertexCapacity. */
#define MVRT_SMOOTH_STEPS_PER_CELL 256
typedef struct mvrt_smooth_params
{
	int32_t iterations;	  /* 0..256, default 4 */
	int32_t weightEven;	  /* -256..256, default 256 */
	int32_t weightOdd;	  /* -256..256, default 256 */
	int32_t limit;		  /* 0..128, default 127 */
	uint32_t reserved[4]; /* 0 */
} mvrt_smooth_params;
/* Fills *p with the defaults above */
int mvrt_smooth_default_params( mvrt_smooth_params* p );
int mvrt_svo_surface_smooth( const mvrt_svo* svo, const uint8_t* masksDev /* NULL: the masks of mvrt_svo_surface_masks */,
							 const mvrt_smooth_params* params /* NULL: the defaults */, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev,
							 uint32_t* indicesDev /* 4 per face */, float* verticesDev /* 3 per vertex */, int32_t* displacementsDev /* 3 per vertex */,
							 uint8_t* neighboursDev /* 1 per vertex */, uint64_t* nFacesOut, uint64_t* nVerticesOut, uint64_t* clampedOut, void* stream );

/* Adopt an SVO built elsewhere (e.g. IntersectorOctree::buildDAGReference on the CPU, IntersectorOctree.hpp:
 * 224-231): nodes in the reference's 68-byte layout, root last.  embeddedMask = 0 selects the variant where
 * the mask is fetched from the node (voxCommon.hpp:353-356; required above 0xFFFFFF nodes). */
/* nVoxelsPSum is used as stored: vIndex = the sum of the stored values along the path (voxCommon.hpp:388-391), whatever they are -- e.g. all zero
 * for buildOctreeNaive's nodes (IntersectorOctree.hpp:195), which then give vIndex 0 like the reference.  (Internally the last level's value is
 * replaced by a popcount of the mask when the upload is found to carry exactly that there, as every octree built by bottomUpOctreeBuild does.)
 * The upload contract, checked on the host by mvrt_svo_check_upload before any GPU work (a rejected upload returns non-zero and leaves the handle
 * exactly as it was; mvrt_last_error names the rule and the first offending node):
 *   1. gridRes is a power of two in [2, 2^21].
 *   2. Every child word of every node, reachable or not, is 0xFFFFFFFF where the mask bit is clear; where it is set, 0xFFFFFFFF (a voxel) or a node
 *      index below numberOfNodes -- embedded: the index in bits 0-23 and that node's mask byte in bits 24-31; plain: the whole word.
 *   3. From the root (the last node) every reachable node has one depth; voxel children occur only in nodes at depth log2(gridRes) - 1, node
 *      children only above it.  This rejects cycles, octrees deeper or shallower than gridRes, nodes shared at two depths and voxels above the
 *      last level (coarse voxels: not supported).
 *   4. The largest nVoxelsPSum sum along a root-to-voxel path (64-bit) is below numberOfVoxels (so a non-empty octree needs numberOfVoxels >= 1).
 *   5. embeddedMask: numberOfNodes < 0xFFFFFF.
 * Accepted and traced like the reference: any numbering with the root last, unreachable nodes, any sharing at one depth, reachable inner nodes with
 * mask 0, any nVoxelsPSum within rule 4, the empty octree (one root of mask 0, numberOfVoxels 0). */
int mvrt_svo_upload( mvrt_svo* svo, const void* nodes68Host, uint32_t numberOfNodes, const void* attribs8Host, uint32_t numberOfVoxels, const float origin[3],
					 float dps, int gridRes, int hasEmission, int embeddedMask, void* stream );
/* The rules above on host arrays alone (no HIP call, no handle): 0 when mvrt_svo_upload would accept them, else non-zero with mvrt_last_error set.
 * For applications that load octrees from files. */
int mvrt_svo_check_upload( const void* nodes68Host, uint32_t numberOfNodes, uint32_t numberOfVoxels, int gridRes, int embeddedMask );

/* Walk whatever octree the handle holds, uploaded or built, and list its voxels (new; an uploaded octree keeps no Morton codes, a walk from the root recovers
 * them).  A path listing: one entry per root-to-voxel path, in ascending path order.  A path, three bits per level with the root's slot highest, is the voxel's
 * Morton code; the paths of a DAG are distinct by construction, so there are no duplicates.  Per entry, into caller device arrays of `capacity` entries:
 *   - xyzDev: 3 x uint32, decoded from the path like mvrt_svo_read_voxels does (x is bit 0 of each 3-bit group).
 *   - vIndexDev: uint32, the stored nVoxelsPSum summed from the root to the voxel: exactly what mvrt_trace_batch reports for a hit on that voxel (upload rule 4
 *     keeps it below numberOfVoxels).
 *   - attribsDev: 8 bytes, the attribute buffer's entry vIndex, copied verbatim, alpha bytes included.
 * Any output pointer may be NULL; all NULL is the sizing call (capacity is then ignored).  The call blocks like mvrt_svo_surface_quads: *nOut, a 64-bit path count,
 * comes back to the host.  On an upload with non-canonical sums it can exceed numberOfVoxels; reachable inner nodes of mask 0 end their path and contribute
 * nothing; the empty octree gives 0 and succeeds.  A capacity below the count is an error: the count is still returned and NOTHING is written to the caller's
 * arrays.  Every flavour is accepted: a handle that keeps Morton codes (every octree this library built, the tree flavour among them) is answered from the codes
 * with vIndex = the entry's number, every other one is walked; the bytes are the same either way.  A handle without an octree is refused ("no octree").  The
 * handle is never modified; a failed allocation of scratch returns an error, leaves the octree whole and leaks nothing. */
int mvrt_svo_walk_voxels( const mvrt_svo* svo, uint64_t capacity, uint32_t* xyzDev, uint32_t* vIndexDev, uint32_t* attribsDev, uint64_t* nOut, void* stream );
/* Make the handle's octree one this library built: walk it (above; a handle that keeps its codes: take its list as it is), bring the attributes into Morton
 * order and build the levels again.  The result is the octree mvrt_svo_build_voxels would build from the walked list with these flags (MVRT_BUILD_NO_DAG |
 * MVRT_BUILD_NO_EMBEDDED_MASK only): same nodes, same numbering, vIndex = Morton rank, cell index and prefix tables present -- after it mvrt_svo_read_voxels,
 * mvrt_svo_edit_voxels and mvrt_svo_surface_* accept the handle.  Two things a voxel-list build would change are kept, so that the scene renders identically:
 * the attribute bytes are copied verbatim (no alpha forcing), and hasEmission stays the handle's current flag (a later edit recomputes it, as documented
 * there).  Grid, origin, dps and emission scale are kept; the build flags become `flags`; totalDumpedVoxels becomes the path count.  On a handle this library
 * built, the call is a change of flavour (DAG to no DAG, embedded to plain or the tree flavour).
 * Refused with the handle unchanged, before anything is replaced: a handle without an octree, an octree of 0 paths, more than 2^32 - 2 paths, unknown flags.
 * A failed allocation before the new octree is adopted leaves the handle unchanged too (the new arrays are built next to the old octree, as by
 * mvrt_svo_build_voxels); one after that leaves it empty (see mvrt_svo_destroy above).  Blocks like mvrt_svo_build.  Through mvrt_pt_intersector( pt ): the steps
 * issued before finish first, as for an edit; the frame buffer is not cleared.  It invalidates every mvrt_device_octree view of the handle. */
int mvrt_svo_rebuild( mvrt_svo* svo, int flags, void* stream );
int mvrt_svo_get_info( const mvrt_svo* svo, mvrt_svo_info* info );
int mvrt_svo_set_emission_scale( mvrt_svo* svo, float scale ); /* m_emissionScale (:273) */
/* bytes of the device structure the traversal and mvrt_svo_download work from (the reference's layout would be numberOfNodes * 68):
 * 64-byte lines per node (+ a 16 MiB prefix table, the 32-byte children arrays and prefix tables the traversal reads and, for octrees built here, the cell index
 * that turns a hit voxel's path into its index: ~25 bytes per voxel) for DAG octrees; for GPU-built octrees WITHOUT node sharing whose masks are not embedded
 * ("tree" flavour: MVRT_BUILD_NO_DAG with >= 0xFFFFFF nodes or MVRT_BUILD_NO_EMBEDDED_MASK) 5 bytes per node + one 16-byte two-level brick
 * per node of every second level (four bricks share a 64-byte line). */
uint64_t mvrt_svo_traversal_bytes( const mvrt_svo* svo );
/* m_nodeBuffer / m_vAttributeBuffer (:265-266): the device arrays.  Attributes are the reference's VoxelAttirb[numberOfVoxels]; nodes are
 * this library's 64-byte lines {u32 children[8]; u32 nVoxelsPSum[8]} (the reference's 68-byte node minus its leading mask word, which rides
 * in bits 24-31 of the parent's pointer); for an octree too large for that (no node sharing, > 2^24 nodes: the tree flavour) they are its 16-byte
 * two-level bricks {u8 childMask[8]; u32 ownMask; u32 base}.  mvrt_svo_info::flavour says which of the three layouts the pointer has; use
 * mvrt_svo_download for the reference layout. */
const void* mvrt_svo_node_buffer_dev( const mvrt_svo* svo );
const void* mvrt_svo_attribute_buffer_dev( const mvrt_svo* svo );
/* read the SVO back in the reference layout (parity checks of build); either pointer may be NULL */
int mvrt_svo_download( const mvrt_svo* svo, void* nodes68Host, void* attribs8Host, uint64_t* mortonHost, void* stream );

/* Host-callable batch form of the device method IntersectorOctreeGPU::intersect (:243-251) ==
 * octreeTraverse_EfficientParametric (voxCommon.hpp:231-423).  SoA device arrays of n floats each.
 * isShadowDev: per-ray flags (nonzero = isShadowRay: vIndex not accumulated) or NULL for "all false".
 * Outputs: t (MVRT_MAX_FLOAT on a miss), nMajor (1:x 2:y 0:z; -1 on a miss), vIndex (0 on a miss / shadow);
 * descentsDev (optional) = child-pointer fetches per ray (voxCommon.hpp:381), the unit of the
 * algorithmic-bytes model in DESIGN.md. */
int mvrt_trace_batch( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
					  const float* rdzDev, const uint8_t* isShadowDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev, uint32_t* descentsDev, void* stream );
/* Same with a START HINT per ray (new; no counterpart in the reference, which starts every ray at the root, voxCommon.hpp:306-312):
 * originVoxelMortonDev[i] = the 3-bits-per-level root->voxel path (= Morton code of the grid cell, x = bit 0) of ANY voxel that exists in the
 * octree, or ~0 for "no hint".  The traversal replays the walk from the root along that path arithmetically for as long as the ray's origin lies
 * in the same octants and starts below the root; every output, descents included, is identical to the unhinted call for every valid hint -- a
 * hint near the origin only makes it cheaper (the path tracer hints each secondary ray with the voxel its path just hit).  Embedded-mask
 * octrees only; ignored otherwise.  A code that names a cell WITHOUT a voxel is an error the library does not detect. */
int mvrt_trace_batch_hinted( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
							 const float* rdzDev, const uint8_t* isShadowDev, const uint64_t* originVoxelMortonDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev,
							 uint32_t* descentsDev, void* stream );
/* The same rays with a DISTANCE LIMIT per ray (new; every ray of the reference runs to infinity).  tMaxDev: n floats, required.  Ray i reports what mvrt_trace_batch
 * reports for it when that hit has t <= tMax[i] -- t is the traversal's own t, in units of rd -- and a miss (MVRT_MAX_FLOAT, -1, 0) otherwise, bit for bit for every
 * ray, the ones with zero direction components included.  A NaN tMax, 0 or a negative one therefore always gives a miss; +inf gives the unlimited result, and so
 * does MVRT_MAX_FLOAT for every hit with a finite t.  The one difference: a ray without a direction (every component zero or denormal) can report a hit at
 * t = +inf, as in the reference; inf <= MVRT_MAX_FLOAT is false, so that ray is a miss under MVRT_MAX_FLOAT and a hit under +inf.
 * The walk ends early once everything still to come is entered beyond the limit (by a margin that covers the rounding of the entry times);
 * descentsDev (optional) = the child fetches the limited ray made: at most those of the unlimited ray, equal to them on a reported hit.
 * Arguments, outputs and asynchrony as for mvrt_trace_batch (nMajorDev, vIndexDev, descentsDev may be NULL).  Embedded and plain flavours, uploaded or built, up to
 * MVRT_DEVICE_MAX_LEVELS levels (the octrees mvrt_svo_device_view accepts: the kernel is the per-thread walk of include/mvrt/device.hpp); the tree flavour is
 * refused by name.  n = 0 succeeds without a launch.  A NULL tMaxDev, tDev or ray array is refused on the host before the handle is looked at. */
int mvrt_trace_batch_range( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
							const float* rdzDev, const uint8_t* isShadowDev, const float* tMaxDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev,
							uint32_t* descentsDev, void* stream );
/* Per-face ambient occlusion of the voxel surface (new; the reference has none).  For every face f of a list (faceVoxel, faceDir) as mvrt_svo_surface_quads /
 * _mesh return it -- any list of (vIndex, direction) pairs is legal -- openDev[f] = how many of `samples` shadow rays leave the face's centre without being
 * occluded within `radius`, under the contract of mvrt_trace_batch_range.
 *   - samples = K, a power of two in [1, 256].  Sample k of direction d has the direction sampleLambertian( a_k, b_k, N_d ) of the path tracer
 *     (renderCommon.hpp:134-151) in the deterministic math of mvrt_detmath.h, at the Hammersley point a_k = (k + 0.5) / K, b_k = the base-2 radical inverse of k
 *     (both exact in fp32); N_d = the unit normal of direction d in the order of mvrt_svo_surface_masks (0 -Y, 1 +Y, 2 -Z, 3 +X, 4 +Z, 5 -X), its zeros +0.0.
 *     mvrt_ao_directions returns that table, dirsHost[(d * K + k) * 3 + axis]: host only, no GPU call.  The bake uses exactly these bits.
 *   - Origin = the face centre.  With the voxel at integer (x, y, z), decoded from its Morton code: c2 = 2 * coord + 1 on the two in-plane axes, 2 * coord (-) or
 *     2 * coord + 2 (+) on the normal axis; ro[a] = lower[a] + (float)c2 * (0.5f * dps), each operation rounded, no FMA.  No offset along the normal: a hit
 *     needs 0 < t, which keeps a ray from hitting the voxel it leaves.
 *   - radius > 0 in the units of dps (the directions have unit length up to rounding); +inf = unlimited (sky visibility), and MVRT_MAX_FLOAT the same for the bake's
 *     own rays, whose directions have unit length: a t of +inf needs a ray without a direction (mvrt_trace_batch_range above).  NaN and values <= 0 are
 *     refused on the host, as are other sample counts and NULL arrays (with nFaces > 0), all before the handle is looked at.
 *   - Handles as for mvrt_svo_surface_quads (an upload is refused: "keeps no Morton codes"; an empty handle: "no octree"), except the tree flavour, which is
 *     refused by name, and octrees above MVRT_DEVICE_MAX_LEVELS levels.  The handle is never modified.
 *   - Every faceVoxel must be below numberOfVoxels and every faceDir below 6: checked on the device BEFORE anything is written.  Otherwise the call fails, names
 *     the lowest offending entry and leaves openDev untouched.
 *   - The call blocks like mvrt_svo_surface_quads.  Its scratch (the direction table) is one allocation: if that fails the call returns an error and leaks nothing. */
int mvrt_ao_directions( int samples, float* dirsHost /* 6 * samples * 3 */ );
int mvrt_svo_surface_ao( const mvrt_svo* svo, uint64_t nFaces, const uint32_t* faceVoxelDev, const uint8_t* faceDirDev, int samples, float radius, uint16_t* openDev /* nFaces */,
						 void* stream );
/* convenience: packed host arrays (n*3 floats), synchronous */
int mvrt_trace_batch_host( const mvrt_svo* svo, uint64_t n, const float* roHost, const float* rdHost, const uint8_t* isShadowHost, float* tHost, int32_t* nMajorHost,
						   uint32_t* vIndexHost, uint32_t* descentsHost );

/* The `render` kernel (voxKernel.cu:437-483) as launched by voxRTGPU.cpp:191-203: one primary ray per pixel
 * through the pixel centre; colour = voxel colour (showVertexColor) or the hit normal.  rgbaDev: width*height
 * uchar4.  Optional per-pixel outputs for parity checks (may be NULL). */
int mvrt_render_primary( const mvrt_svo* svo, const float camera[15], int width, int height, int showVertexColor, uint8_t* rgbaDev, float* tDev, int32_t* nMajorDev,
						 uint32_t* vIndexDev, uint32_t* descentsDev, void* stream );

/* Device view of an octree: the by-value IntersectorOctreeGPU a user kernel takes (IntersectorOctreeGPU.hpp:243-275), for the
 * per-thread traversal of include/mvrt/device.hpp (mvrt::DeviceOctree).  Fixed-width fields only; pointers are device addresses
 * stored as uint64_t.
 *   - The view is a SNAPSHOT of the handle: any later build (mvrt_svo_build_voxels included), mvrt_svo_edit_voxels, mvrt_svo_rebuild, upload, cleanUp or
 *     destroy of that handle invalidates it (its buffers are freed, replaced or rewritten, hasEmission may change), exactly like a copy of
 *     the reference's struct.  Take a new view after each of them.
 *   - emissionScale is copied from the handle; the caller may edit it in the copy it holds (getVoxelEmission( v, true ) uses it).
 *   - Flavours MVRT_FLAVOUR_EMBEDDED and MVRT_FLAVOUR_PLAIN only; tree-flavour octrees are refused.
 *   - levels <= MVRT_DEVICE_MAX_LEVELS (the depth of the per-thread stack). */
#define MVRT_DEVICE_MAX_LEVELS 16
typedef struct mvrt_device_octree
{
	uint32_t structBytes; /* sizeof( mvrt_device_octree ) of the library that filled it */
	uint32_t flavour;	  /* MVRT_FLAVOUR_* */
	uint64_t nodes;		  /* 64-byte lines {children[8], nVoxelsPSum[8] (embedded) or the 8 child masks (plain)} */
	uint64_t kids;		  /* embedded: children[8] per node, 32 bytes per node (0 = read them from the node lines) */
	uint64_t masks;		  /* per-node own mask, one byte per node */
	uint64_t psumCold;	  /* plain: nVoxelsPSum[node * 8 + child] */
	uint64_t attrs;		  /* VoxelAttirb[numberOfVoxels]: {uchar4 color, uchar4 emission} */
	uint64_t cellBlocks;  /* reserved for the cell index of octrees built by the library (0 = none); the traversal walks nVoxelsPSum */
	uint64_t cellEntries;
	float lower[3];
	float upper[3];
	float dps;
	float emissionScale;
	uint32_t hasEmission;
	uint32_t levels;
	uint32_t numberOfNodes;
	uint32_t numberOfVoxels;
	uint32_t rootIndex; /* numberOfNodes - 1 */
	uint32_t rootMask;	/* the root's own occupancy mask */
	uint32_t treeRoot;	/* 0 (tree flavour only) */
	uint32_t cellBits;
} mvrt_device_octree;
#ifdef __cplusplus
#define MVRT_STATIC_ASSERT_( c, m ) static_assert( c, m )
#else
#define MVRT_STATIC_ASSERT_( c, m ) _Static_assert( c, m )
#endif
MVRT_STATIC_ASSERT_( sizeof( mvrt_device_octree ) == 128, "mvrt_device_octree is 128 bytes" );
MVRT_STATIC_ASSERT_( __builtin_offsetof( mvrt_device_octree, nodes ) == 8 && __builtin_offsetof( mvrt_device_octree, cellEntries ) == 56 &&
						 __builtin_offsetof( mvrt_device_octree, lower ) == 64 && __builtin_offsetof( mvrt_device_octree, emissionScale ) == 92 &&
						 __builtin_offsetof( mvrt_device_octree, levels ) == 100 && __builtin_offsetof( mvrt_device_octree, cellBits ) == 124,
					 "mvrt_device_octree field offsets" );
/* Fill *out with the device view of svo (no GPU call).  Fails without an octree, on a tree-flavour octree and above MVRT_DEVICE_MAX_LEVELS. */
int mvrt_svo_device_view( const mvrt_svo* svo, mvrt_device_octree* out );

/* ---- Level of detail per ray inside ONE octree (new; the reference has none) ----------------------------------------------------------
 * The attribute pyramid.  mvrt_svo_lod_prepare attaches to the handle, for every level L in [1, levels - 1], the occupied cells of that level as ascending codes
 * (uint64, the Morton code of any voxel below the cell >> 3 * ( levels - L )), their 8-byte attributes and their voxel counts (uint32): exactly what
 * mvrt_svo_coarse_voxels( levelsDown = levels - L, minCount = 1 ) lists, in its order, from the same exact integer sums over the voxels (never means of means).
 * The pyramid is keyed by the cell's code, not by the node: the octree is a DAG, subtrees of equal shape share nodes whatever their colours.
 *   - Handles as for mvrt_svo_coarse_voxels (an upload is refused: "keeps no Morton codes"; an empty handle: "no octree"), except the tree flavour, which is
 *     refused by name, and octrees above MVRT_DEVICE_MAX_LEVELS levels.  A one-level octree has an empty pyramid and succeeds.
 *   - The call blocks.  It is built on the GPU from the sorted voxel list; nothing travels to the host.  A failed allocation leaves the octree whole, no
 *     half-built pyramid and no leak.  A second call replaces the pyramid.
 *   - Every build, edit (attribute-only ones included, and an edit the device checks refuse as well: it is dropped before the edit runs), rebuild, upload, coarsen
 *     in place, every other in-place voxel-set call that changes the handle, cleanUp and destroy drops the pyramid: it never outlives the voxels it describes.
 *     mvrt_svo_lod_release drops it by hand; mvrt_svo_lod_bytes = its size (0 without one).
 * mvrt_device_lod is the by-value view for application kernels (mvrt::DeviceLod, include/mvrt/device.hpp): entry L of each array describes level L; entry
 * `levels` is the voxel list itself (its codes, the octree's attributes, numberOfVoxels; no counts), entry 0 and the entries above `levels` are 0.  Like
 * mvrt_device_octree it is a snapshot: whatever drops the pyramid invalidates it. */
typedef struct mvrt_device_lod
{
	uint32_t structBytes; /* sizeof( mvrt_device_lod ) of the library that filled it */
	uint32_t levels;	  /* of the octree */
	uint64_t codes[MVRT_DEVICE_MAX_LEVELS + 1];		 /* per level: ascending cell codes (uint64) */
	uint64_t attrs[MVRT_DEVICE_MAX_LEVELS + 1];		 /* per level: {uchar4 color, uchar4 emission} per cell */
	uint64_t cellVoxels[MVRT_DEVICE_MAX_LEVELS + 1]; /* per level: voxels per cell (uint32); 0 at level `levels` */
	uint32_t count[MVRT_DEVICE_MAX_LEVELS + 1];		 /* per level: the number of cells */
	uint32_t reserved;
} mvrt_device_lod;
MVRT_STATIC_ASSERT_( sizeof( mvrt_device_lod ) == 488, "mvrt_device_lod is 488 bytes" );
MVRT_STATIC_ASSERT_( __builtin_offsetof( mvrt_device_lod, codes ) == 8 && __builtin_offsetof( mvrt_device_lod, attrs ) == 144 &&
						 __builtin_offsetof( mvrt_device_lod, cellVoxels ) == 280 && __builtin_offsetof( mvrt_device_lod, count ) == 416,
					 "mvrt_device_lod field offsets" );
#undef MVRT_STATIC_ASSERT_
int mvrt_svo_lod_prepare( mvrt_svo* svo, void* stream );
int mvrt_svo_lod_release( mvrt_svo* svo );
uint64_t mvrt_svo_lod_bytes( const mvrt_svo* svo );
/* Fill *out with the view of the pyramid (no GPU call).  Fails without a prepared pyramid. */
int mvrt_svo_lod_view( const mvrt_svo* svo, mvrt_device_lod* out );
/* CONE-LIMITED rays: ray i stops the octree walk at its own level of detail.  coneADev, coneBDev: n floats each, required; the ray's footprint at time S is
 * f = coneA + coneB * S (one fp32 product, one fp32 sum, each rounded).  On the first visit of an inner node at level in [1, levels - 1], entered at time S, the
 * node is terminal iff 0 < S and dps * 2^( levels - level ) <= f, and reports the hit a voxel in its place would: t = S, nMajor by the voxel's rule,
 * levelDev[i] = the node's level, cellCodeDev[i] = the cell's code (as in the pyramid above).  A voxel hit reports level = levels and the voxel's Morton code, a miss
 * MVRT_MAX_FLOAT, -1, 0, 0.  The root is never terminal.  Bit for bit: t and nMajor of a walk stopped at level D are those of mvrt_trace_batch against the octree
 * mvrt_svo_coarsen makes with levelsDown = levels - D; a zero, negative or NaN footprint gives mvrt_trace_batch's t, nMajor and descents; descents never exceed the
 * unlimited ray's; where the unlimited ray hits the cone ray hits too, and it may hit where that one misses (a coarse cell is solid to it).
 *   - indexDev (uint32: the cell's rank in its level; at a voxel the vIndex) and attribDev (8 bytes per ray: the pyramid's attribute of the cell, at a voxel the
 *     voxel's; zeros on a miss) need a prepared pyramid (mvrt_svo_lod_prepare): without one they are refused by name when non-NULL.  Without them any octree
 *     mvrt_svo_device_view accepts is legal, uploads included.  nMajorDev, levelDev, cellCodeDev, indexDev, attribDev, descentsDev may be NULL.
 *   - Asynchrony as for mvrt_trace_batch_range; the tree flavour is refused by name.  n = 0 succeeds without a launch.  A NULL coneADev, coneBDev, tDev or ray array
 *     is refused on the host before the handle is looked at. */
int mvrt_trace_batch_cone( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
						   const float* rdzDev, const float* coneADev, const float* coneBDev, float* tDev, int32_t* nMajorDev, uint32_t* levelDev, uint64_t* cellCodeDev,
						   uint32_t* indexDev, uint32_t* attribDev /* 2 per ray */, uint32_t* descentsDev, void* stream );
/* mvrt_render_primary with one cone per pixel: the rays of mvrt_render_primary (CameraPinhole::shoot through pixel centres), coneA = 0 and
 * coneB = lodScale * ( ( 2.0f * tanHthetaY ) / (float)height ), computed once on the host in that order: lodScale pixels' width at rd . front = 1.  Colour = the
 * terminal cell's pyramid colour, or the voxel's at a voxel, converted as mvrt_render_primary converts a voxel colour (showVertexColor: needs a prepared pyramid), or
 * the hit normal.  levelDev: the level each pixel stopped at (0 on a miss).  lodScale = 0 equals mvrt_render_primary in rgba, t, nMajor and descents.  The kernel
 * is the per-thread walk: octrees as for mvrt_trace_batch_cone.  rgbaDev, tDev, nMajorDev, levelDev, descentsDev may be NULL. */
int mvrt_render_primary_lod( const mvrt_svo* svo, const float camera[15], int width, int height, float lodScale, int showVertexColor, uint8_t* rgbaDev, float* tDev,
							 int32_t* nMajorDev, uint32_t* levelDev, uint32_t* descentsDev, void* stream );

/* CameraPinhole::initFromPerspective (renderCommon.hpp:21-35) */
int mvrt_camera_from_matrices( const float view[16], const float proj[16], float focus, float lensR, float cameraOut[15] );

/* Stable stream compaction (StreamCompaction::filter semantics, StreamCompaction.hpp:87-184): for n device
 * flags, dstIndexDev[i] = number of kept items before i (0xFFFFFFFF if dropped), *keptDev = kept count.
 * Same wave64 ballot + ordered block scan the path tracer uses for live rays. */
int mvrt_compact_indices( const uint8_t* keepDev, uint64_t n, uint32_t* dstIndexDev, uint32_t* keptDev, void* stream );

/* ---- PathTracer ---------------------------------------------------------------------------- */
int mvrt_pt_create( mvrt_pt** out );
int mvrt_pt_destroy( mvrt_pt* pt );				/* PathTracer::cleanUp, PathTracer.hpp:71-79 */
/* PathTracer::setup (:43-69): PMJ02 table (pmjSampler.hpp:114-144) and work buffers.  The reference's kernel
 * path / include dir / isNvidia arguments have no meaning here (no runtime compilation). */
int mvrt_pt_setup( mvrt_pt* pt, void* stream );
/* read back PMJSampler::m_samples (pmjSampler.hpp:114-144): 128 sequences x 4096 float2 = 4 MiB */
int mvrt_pt_download_pmj( mvrt_pt* pt, float* tableHost );
int mvrt_pt_resize_framebuffer_if_needed( mvrt_pt* pt, void* stream, int width, int height ); /* :81-97 */
int mvrt_pt_clear_framebuffer( mvrt_pt* pt, void* stream );									 /* :98-102, steps = 0 */
/* PathTracer::loadHDRI (:104-116) + HDRI::load/loadPrimary (renderCommon.hpp:214-326): decoded float4 pixels.
 * rgbaPrimaryHost may be NULL (then primary lookups use the lighting map's pixels AND size -- the reference
 * would read out of bounds, renderCommon.hpp:356-363).  A failed load leaves the map loaded before, or none, fully in place.
 * Refused before any pointer is read or anything is allocated: a non-NULL primary with widthPrimary <= 0 or heightPrimary <= 0, and a lighting or
 * primary map of 2^31 pixels or more (pixels are indexed with 32-bit integers).
 * Zero tables (a second deviation): an importance table whose f64 total is not > 0 -- an all-black map, the -y table of a sky over a black ground,
 * the tables of a 1x1 / 2x1 / 1x2 map whose axis no pixel centre faces -- is stored as all zeros; the reference normalises by the total and converts
 * NaN to u32, which is undefined (voxKernel.cu:600-608).  Such a table selects nothing: where the hit normal picks it, next-event estimation
 * returns L = 0 with pdf = 1 along the normal, so the contribution is exactly 0, the shadow ray is still traced (along the normal), the four sample
 * dimensions are still consumed and the rest of the path is unchanged.  The reference would divide by zero in its row search and index about 2^32
 * elements outside the table (renderCommon.hpp:367-435).  Maps without such a table are unaffected, bit for bit. */
int mvrt_pt_load_hdri( mvrt_pt* pt, void* stream, const float* rgbaHost, int width, int height, const float* rgbaPrimaryHost, int widthPrimary, int heightPrimary );
/* same from Radiance .hdr files (RGBE, flat or RLE; value = c * 2^(E-136)); filePrimary may be NULL */
int mvrt_pt_load_hdri_file( mvrt_pt* pt, void* stream, const char* file, const char* filePrimary );
/* host-only: decode a Radiance .hdr file to float4 pixels (alpha 1) exactly as mvrt_pt_load_hdri_file does -- flat and new-RLE scanlines,
 * value = c * 2^(E-136).  rgbaHost may be NULL to query the size. */
int mvrt_rgbe_read_file( const char* file, float* rgbaHost, uint64_t capacityPixels, int* width, int* height );
/* read back one importance table (parity checks): which = 0 uniform, 1..6 = +x,-x,+y,-y,+z,-z; width*height u32 */
int mvrt_pt_download_hdri_sat( mvrt_pt* pt, int which, uint32_t* satHost );
int mvrt_pt_set_hdri_scale( mvrt_pt* pt, float scale ); /* HDRI::m_scale = 1.75 (renderCommon.hpp:480); <= 0 disables NEE */
/* PathTracer::updateScene (:139-148) -> IntersectorOctreeGPU::build */
int mvrt_pt_update_scene( mvrt_pt* pt, const float* verticesHost, const float* vcolorsHost, const float* vemissionsHost, uint64_t nVertices, void* stream,
						  const float origin[3], float dps, int gridRes );
mvrt_svo* mvrt_pt_intersector( mvrt_pt* pt ); /* &PathTracer::m_intersectorOctreeGPU (:18); owned by pt */
/* PathTracer::step (:150-169): one launch of renderPT semantics = 16 spp for every pixel, iteration = steps++.
 * Wavefront implementation: generate -> [trace -> count/scan -> shade+compact] x <= 9 -> accumulate. */
int mvrt_pt_step( mvrt_pt* pt, void* stream, const float camera[15] );
/* same with the matrices GetCameraMatrix produces in the reference (:152-156) */
int mvrt_pt_step_matrices( mvrt_pt* pt, void* stream, const float view[16], const float proj[16], float focus, float lensR );
/* Consecutive step() calls are pipelined on internal streams (`depth` steps in flight, default 2; 1 = none) so that
 * the thin late bounces of one step overlap the dense early bounces of the next.  Results are unchanged (frame-buffer
 * additions are chained in step order).  Every call that consumes the frame buffer (resolve, to_image, read, clear)
 * first makes `stream` wait for the steps in flight; callers that read mvrt_pt_framebuffer_dev() themselves call
 * mvrt_pt_join( pt, stream ) before. */
int mvrt_pt_set_pipeline_depth( mvrt_pt* pt, int depth );
/* Secondary rays (shadow, extra, bounce) start below the root, hinted with the voxel their path hit last (mvrt_trace_batch_hinted); default on.
 * 0 = every ray walks from the root like the reference's.  Results are identical either way. */
int mvrt_pt_set_origin_hints( mvrt_pt* pt, int enable );
/* step() is DEFERRED: up to maxSteps (1 = launch immediately; 0 = automatic, the default: about two full-HD steps of samples per pass and at most half of the caller's
 * frame -- the steps between its last two clear_framebuffer calls --, so that a frame is at least two passes that overlap) consecutive step() calls are merged into one
 * wavefront pass -- larger launches, identical per-sample results, additions to the frame buffer still step by step.
 * Any consumer (resolve, to_image, read, clear, join, get_stats ...) launches what is pending first. */
int mvrt_pt_set_batch_steps( mvrt_pt* pt, int maxSteps );
/* A SMALL pass (<= 40 M samples: a tile share of a multi-GPU frame, a small frame) of >= 2 merged steps is launched as two sibling
 * passes on two internal streams, so that the launch tails and the shading of one overlap with the traversal of the other
 * (default on; needs pipeline depth >= 2).  Results are unchanged. */
int mvrt_pt_set_split_small_passes( mvrt_pt* pt, int enable );
int mvrt_pt_join( mvrt_pt* pt, void* stream );
int mvrt_pt_resolve( mvrt_pt* pt, void* stream );						/* :130-137, renderResolve */
int mvrt_pt_to_image_async( mvrt_pt* pt, void* stream, uint8_t* rgbaHost ); /* :118-129 resolve + DtoH (caller syncs) */
int mvrt_pt_get_steps( const mvrt_pt* pt );								/* :33 */
uint64_t mvrt_pt_get_number_of_voxels( const mvrt_pt* pt );				/* :34-37 */
uint64_t mvrt_pt_get_octree_bytes( const mvrt_pt* pt );					/* :38-41 (nodes * 68) */
/* F32 accumulation buffer (m_frameBufferF32, :22): float4 per OWNED pixel, xyz = sum, w = spp */
int mvrt_pt_read_framebuffer( mvrt_pt* pt, void* stream, float* rgbaHost /* ownedPixels*4 */ );
float* mvrt_pt_framebuffer_dev( mvrt_pt* pt );
uint8_t* mvrt_pt_framebuffer_u8_dev( mvrt_pt* pt );

/* First-hit feature buffers for denoising, compositing, picking (new; the reference has none).  Two more accumulation buffers beside the frame
 * buffer: float4 per OWNED pixel, the frame buffer's compact layout, padding and stride, cleared with it by clear_framebuffer and reallocated with
 * it by resize_framebuffer_if_needed / set_tile.  They describe the hit of each sample's PRIMARY ray -- the jittered thin-lens ray step() generates
 * for it, not a pixel-centre ray, so they match the beauty image at silhouettes and with lensR > 0:
 *   MVRT_AOV_ALBEDO        xyz = sum of the hit voxel's colour (channel / 255.0f), w = number of samples whose primary ray hit
 *   MVRT_AOV_NORMAL_DEPTH  xyz = sum of the hit face's axis normal (+-1 on one axis), w = sum of the hit's t
 * t is what mvrt_trace_batch returns for that ray, whose direction is not normalised: for this camera rd . front = focus, so t * focus is the
 * distance along the view axis.  A sample whose primary ray misses adds nothing; the sample count is the frame buffer's w and is not stored again:
 * means are sum / frameBuffer.w (over all samples) or sum / albedo.w (over the hits).  The summation order is fixed like the frame buffer's
 * (per step the 16 samples in ascending order from +0, then steps in issue order); batching, pipelining, tiles, the HDRI scale, emission and
 * origin hints change no bit.  mvrt_pt_assemble_tiles, mvrt_memcpy_d2d and an all-gather apply to them as to the frame buffer;
 * mvrt_resolve_buffer is NOT meant for them (it divides by w and tone-maps).
 * Off by default: with them off every launch, allocation and output is that of a library without them.  On: 32 bytes per pixel and merged step of
 * path state, 32 bytes per pixel of buffers, two small kernels per pass. */
#define MVRT_AOV_ALBEDO 0
#define MVRT_AOV_NORMAL_DEPTH 1
/* Waits for the steps in flight, then allocates or frees.  Fails, handle unchanged, while steps are accumulated (get_steps != 0: the buffers would
 * not match the frame buffer's sample count) -- clear_framebuffer first.  May be called before or after resize_framebuffer_if_needed.  If the
 * path state no longer fits, the handle has NO frame afterwards, like after any failed reallocation (mvrt_pt_set_test_free_bytes). */
int mvrt_pt_set_aovs( mvrt_pt* pt, int enable );
/* NULL (and mvrt_last_error) when off, without a frame or for another `which`; callers reading it on their own stream call mvrt_pt_join before */
float* mvrt_pt_aov_dev( mvrt_pt* pt, int which );
/* host copy; waits for the steps in flight like mvrt_pt_read_framebuffer */
int mvrt_pt_read_aov( mvrt_pt* pt, void* stream, int which, float* rgbaHost /* ownedPixels*4 */ );

/* Luminance moments, the per-pixel variance a denoiser needs (new; the reference has none).  One more accumulation buffer with the frame buffer's layout,
 * padding and stride, cleared and reallocated with it: float4 per OWNED pixel, x = sum of l, y = sum of l * l over all samples, z = w = 0 (reserved), with
 *   l = ( 0.2126f * r + 0.7152f * g ) + 0.0722f * b
 * of the sample's radiance, the very value the frame buffer sums.  Order, fp32 without contraction: per pixel and step s1 = sum of l and s2 = sum of l * l
 * (the product rounded, then added) over the 16 samples in ascending order from +0; then x += s1, y += s2, steps in issue order.  Batching, pipelining,
 * sibling passes, tiles and origin hints change no bit.  mvrt_pt_assemble_tiles, mvrt_memcpy_d2d and an all-gather apply as to the frame buffer.
 * The sample variance of the pixel mean's luminance is max( y / n - ( x / n )^2, 0 ) / max( n - 1, 1 ) with n = frameBuffer.w.
 * Independent of mvrt_pt_set_aovs and under the same rules: the call waits for the steps in flight, fails with the handle unchanged while get_steps != 0,
 * may come before or after resize_framebuffer_if_needed, and leaves NO frame when the path state no longer fits.  Off by default: with it off every launch,
 * allocation and output is that of a library without it.  On: 16 bytes per pixel, one small kernel per pass behind the frame-buffer addition. */
int mvrt_pt_set_moments( mvrt_pt* pt, int enable ); /* new; the reference has none */
/* new; the reference has none.  NULL (and mvrt_last_error) when off or without a frame; callers reading it on their own stream call mvrt_pt_join before */
float* mvrt_pt_moments_dev( mvrt_pt* pt );
/* new; the reference has none.  Host copy; waits for the steps in flight like mvrt_pt_read_framebuffer */
int mvrt_pt_read_moments( mvrt_pt* pt, void* stream, float* rgbaHost /* ownedPixels*4 */ );

/* Denoiser (new; the reference has none): an edge-avoiding a-trous wavelet filter on the demodulated mean radiance, guided by the first-hit feature
 * buffers and by the per-pixel variance of the moments.  Inputs are FULL-FRAME buffers, pixel = y * width + x, float4 each: the frame buffer (color), the two
 * feature buffers and the moments -- of a handle with tileCount == 1 as they are, of tile shares after mvrt_pt_assemble_tiles.  Inputs are not modified.
 * Output: float4 per pixel, xyz = denoised mean radiance, w = 1, so that mvrt_resolve_buffer( out, width * height, u8 ) tone-maps it.
 *
 * THE FILTER.  All arithmetic is fp32 in exactly this order, without contraction; exp is mvrt_exp (mvrt_detmath.h); division and sqrt are IEEE;
 * lum( x ) = ( 0.2126f * x.r + 0.7152f * x.g ) + 0.0722f * x.b; max( a, b ) = a < b ? b : a.
 * Prepare, per pixel, with n = color.w and h = albedo.w:
 *   n == 0: out = (0,0,0,0); the pixel is never filtered and never a tap.
 *   c = color.xyz / n
 *   h == 0 (sky): out = ( c, 1 ) exactly; the pixel is never filtered and never a tap.
 *   A_k = max( ( albedo_k + ( n - h ) ) / n, albedoFloor )  per channel (misses count as albedo 1); with MVRT_DENOISE_NO_DEMODULATION A = (1,1,1)
 *   u = c / A;  N = normalDepth.xyz / n;  Z = normalDepth.w / h;  f = h / n
 *   m1 = moments.x / n;  m2 = moments.y / n;  var = max( m2 - m1 * m1, 0 ) / max( n - 1, 1 );  lA = lum( A );  v = var / ( lA * lA )
 * Iteration i = 0 .. iterations - 1, stride s = 2^i, for every pixel p = (x, y) with n > 0 and h > 0, reading the { u, v } the previous iteration wrote:
 *   lp = lum( u_p );  sv = sigmaLuminance * sqrt( v_p ) + 1e-6f;  acc = (0,0,0), accv = 0, ws = 0
 *   taps dy = -2 .. 2 (outer loop), dx = -2 .. 2 (inner loop), q = ( x + dx * s, y + dy * s ); a tap is skipped when q lies outside the frame or n_q == 0 or h_q == 0:
 *     d = N_p - N_q;  e = ( ( d.x * d.x + d.y * d.y ) + d.z * d.z ) / ( sigmaNormal * sigmaNormal )
 *     dz = ( Z_p - Z_q ) / ( sigmaDepth * max( max( Z_p, Z_q ), 1e-20f ) );  e = e + dz * dz
 *     df = ( f_p - f_q ) / sigmaCoverage;  e = e + df * df
 *     e = e + |lp - lum( u_q )| / sv
 *     w = ( k[dy] * k[dx] ) * mvrt_exp( -e )   with k = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f }
 *     acc_k = acc_k + w * u_q,k;  accv = accv + ( w * w ) * v_q;  ws = ws + w
 *   u'_p = acc / ws;  v'_p = accv / ( ws * ws )     (the centre tap is always present: ws > 0)
 * Finish: out.xyz = u * A with the u of the last iteration, out.w = 1.  The variance is not pre-blurred. */
#define MVRT_DENOISE_NO_DEMODULATION 1u
typedef struct mvrt_denoise_params
{
	uint32_t structBytes;	/* sizeof( mvrt_denoise_params ) */
	int32_t iterations;		/* 1..8, default 5 */
	float sigmaNormal;		/* 0.5  */
	float sigmaDepth;		/* 0.05 */
	float sigmaCoverage;	/* 0.25 */
	float sigmaLuminance;	/* 2.0  */
	float albedoFloor;		/* 0.01 */
	uint32_t flags;			/* MVRT_DENOISE_NO_DEMODULATION */
	uint32_t reserved[2];	/* 0 */
} mvrt_denoise_params;
/* new; the reference has none.  Fills *p with the defaults above (structBytes included) */
int mvrt_denoise_default_params( mvrt_denoise_params* p );
/* new; the reference has none.  Bytes of scratch mvrt_denoise_buffers needs for a frame (0 and mvrt_last_error for a bad size); no GPU call */
uint64_t mvrt_denoise_scratch_bytes( int width, int height );
/* new; the reference has none.  The filter on full-frame device buffers, asynchronous on `stream`; params NULL = the defaults.  outDev: width * height float4; it and
 * scratchDev must not overlap the inputs.  Every rejected argument (structBytes, iterations outside 1..8, a sigma or the floor not greater than 0, a sigma or
 * the floor that is not finite, a sigmaNormal whose square underflows to 0, width or height not greater than 0, scratch too small, a null pointer) fails on the
 * host before any GPU call.
 * Non-finite INPUT is not refused: the filter applies the arithmetic above to it.  What is promised then: a pixel farther than 2 * ( 2^iterations - 1 ) from every
 * non-finite pixel in both x and y (the reach of the taps) gets the value it would get without it, bit for bit; which of the pixels within the reach come out
 * non-finite follows from the arithmetic above (IEEE rules for inf and NaN, a comparison with NaN is false), but payload and sign of a NaN are not part of the contract. */
int mvrt_denoise_buffers( const float* colorDev, const float* albedoDev, const float* normalDepthDev, const float* momentsDev, int width, int height,
						  const mvrt_denoise_params* params, float* outDev, void* scratchDev, uint64_t scratchBytes, void* stream );
/* new; the reference has none.  The same on a handle with tileCount == 1, feature buffers and moments on and at least one step: like resolve it launches the pending steps
 * and makes `stream` wait for the steps in flight; otherwise asynchronous on `stream`.  The handle owns the output and the scratch (kept between calls,
 * released by a resize and by set_tile); an allocation that fails leaves the frame, the accumulated steps and the feature buffers intact and NO denoised
 * buffer.  The frame buffer, the feature buffers, the moments and get_steps are untouched: stepping afterwards continues the accumulation bit-identically.
 * A handle with tileCount > 1 is refused (assemble the shares and call mvrt_denoise_buffers), as are feature buffers or moments off and a frame without steps. */
int mvrt_pt_denoise( mvrt_pt* pt, void* stream, const mvrt_denoise_params* params /* NULL = defaults */ );
/* new; the reference has none.  NULL before the first denoise, after a resize that reallocates, after set_tile and after a denoise whose allocation failed (a call
 * refused for its arguments leaves the image of the last one); read it on the stream the denoise ran on */
float* mvrt_pt_denoised_dev( mvrt_pt* pt );
/* new; the reference has none.  Host copy on `stream` (the stream of the denoise), synchronous */
int mvrt_pt_read_denoised( mvrt_pt* pt, void* stream, float* rgbaHost /* width*height*4 */ );

/* Adaptive sampling (new; the reference has none): a per-pixel SAMPLE MASK restricts the steps to a subset of the owned pixels, and an ERROR MASK computed from
 * the moments says which pixels have not converged.  A sample's radiance depends only on (global pixel, iteration, spp), so for an ACTIVE pixel a step under a
 * mask makes exactly the additions an unmasked step makes -- to the frame buffer (w += 16 included), to both feature buffers and to the moments, same values,
 * same order -- and for an INACTIVE pixel no bit of any buffer changes.  get_steps and the iteration advance as before: a pixel that sits out iteration k never
 * gets iteration k's samples.  Batching, pipelining, sibling passes, tiles, origin hints and the HDRI scale change no bit, and a mask with every valid pixel
 * active equals no mask.  Off by default: with no mask set every launch, allocation and output is that of a library without it.
 *
 * mvrt_pt_set_sample_mask: maskDev holds one byte per owned pixel in the handle's local pixel order (the order of mvrt_pt_framebuffer_dev), nonzero = active;
 * only the first validOwnedPixels bytes are read, padding is never active.  The mask is a snapshot: the call launches the pending steps (they run under the
 * mask they were issued under), lists the active pixels in ascending order, blocks until their number is on the host (*nActiveOut) and the array may be
 * reused.  With no active pixel the call succeeds and the steps that follow advance the counter and launch nothing.  Under a mask everything indexed by task uses
 * the compact numbering: sample = ( ( step * nActive + slot ) * 16 + spp ), slot = the pixel's rank among the active ones -- mvrt_pt_read_sample_radiance,
 * mvrt_pt_sample_radiance_dev, mvrt_pt_read_debug_stage -- and mvrt_pt_stats.samples counts the active samples only.
 * The mask goes off with maskDev == NULL, with mvrt_pt_clear_framebuffer (a new frame needs every pixel), with a resize that reallocates, with mvrt_pt_set_tile
 * and with anything that leaves the handle without a frame; mvrt_pt_update_scene and edits through mvrt_pt_intersector keep it.
 * Refused on the host with the handle unchanged: a null pt, no frame ("no frame buffer").  Every non-NULL call builds its list (one uint32 per owned pixel,
 * kept with the frame) and its scratch aside: when an allocation fails, the call returns an error, the mask that was in force stays in force and nothing leaks. */
int mvrt_pt_set_sample_mask( mvrt_pt* pt, void* stream, const uint8_t* maskDev /* ownedPixels bytes; NULL = off */, uint64_t* nActiveOut /* may be NULL */ ); /* new; the reference has none */
/* new; the reference has none.  The pixels a step samples: validOwnedPixels when no mask is set; 0 without a frame */
uint64_t mvrt_pt_active_pixels( const mvrt_pt* pt );
/* new; the reference has none.  Like resolve it launches the pending steps and makes `stream` wait for the steps in flight; writes one byte (0 or 1) per owned
 * pixel to maskDev (padding 0), blocks and returns the number of ones.  It does NOT set the mask: the caller may combine or grow it first.  Needs a frame and the
 * moments (mvrt_pt_set_moments).  All arithmetic is fp32 in exactly this order, without contraction, division and sqrt IEEE, max( a, b ) = a < b ? b : a.
 * Per pixel, n = frameBuffer.w:
 *   n < (float)minSamples: 1 (n == 0 among them)
 *   otherwise maxSamples > 0 and n >= (float)maxSamples: 0
 *   otherwise m1 = moments.x / n;  m2 = moments.y / n;  var = max( m2 - m1 * m1, 0 ) / max( n - 1, 1 ) (the denoiser's var);  se = sqrt( var );
 *             1 if and only if se > threshold * max( m1, lumFloor )
 * Refused on the host: threshold or lumFloor not greater than 0 (NaN included), minSamples < 1, maxSamples < 0, a null pt or maskDev, moments off, no frame. */
int mvrt_pt_error_mask( mvrt_pt* pt, void* stream, float threshold, float lumFloor, int minSamples, int maxSamples /* 0 = none */, uint8_t* maskDev /* ownedPixels bytes */,
						uint64_t* nActiveOut /* may be NULL */ );

/* Multi-GPU tile split (new; the reference has no multi-GPU path).  The frame is cut into the reference's own
 * 256-pixel blocks (RENDER_NUMBER_OF_THREAD, renderCommon.hpp:13) dealt round-robin: this handle renders blocks
 * b with b % tileCount == tileIndex.  Owned pixels are stored compactly in block order.  Call before
 * resize_framebuffer.  Samples depend only on (global pixel index, spp), so any split reproduces the 1-GPU image.
 * The call leaves the handle WITHOUT a frame, in the state a failed reallocation leaves: everything sized for the old tiling is
 * released at once (both frame buffers, feature buffers, moments, denoised image, path state), the entry points that read a
 * frame report "no frame buffer", mvrt_pt_framebuffer_u8_dev and mvrt_pt_sample_radiance_dev return NULL and
 * mvrt_pt_owned_pixels 0, until the next resize_framebuffer.  The options (set_aovs, set_moments, ...) are kept. */
int mvrt_pt_set_tile( mvrt_pt* pt, int tileIndex, int tileCount );
uint64_t mvrt_pt_owned_pixels( const mvrt_pt* pt ); /* padded to whole 256-pixel blocks */
/* scatter gathered per-rank buffers (rank-major, each rankStridePixels float4) back to a width*height frame */
int mvrt_pt_assemble_tiles( const float* gatheredDev, int tileCount, uint64_t rankStridePixels, int width, int height, float* frameDev, void* stream );
/* renderResolve (voxKernel.cu:779-795) on an arbitrary float4 buffer: per channel mean = x / w, v = 255 * mvrt_pow( mean, 1.0f / 2.2f ) + 0.5f, byte = v
 * truncated, at most 255; alpha = 255.  Outside the ordinary range (deviation: the reference converts v to int before it clamps, which is undefined there):
 *   a mean that is NaN, negative or zero -- 0 / 0 among them, so a pixel without samples is black -- gives 0 (mvrt_pow is 0 for them);
 *   every mean with v >= 255 gives 255, +inf and x / 0 with x > 0 included: the clamp is taken in float, no out-of-range value is ever converted. */
int mvrt_resolve_buffer( const float* rgbaF32Dev, uint64_t nPixels, uint8_t* rgbaU8Dev, void* stream );

/* Per-sample radiance of the LAST step (debug / parity): ownedPixels*16*3 floats on the device */
const float* mvrt_pt_sample_radiance_dev( mvrt_pt* pt );
/* host copy of the x, y, z planes (nSamples floats each) of the last pass; sample = (step * pixels + pixel) * 16 + spp */
int mvrt_pt_read_sample_radiance( mvrt_pt* pt, float* xyzHost, uint64_t nSamples );

/* Debug capture (parity of the live-path compaction, StreamCompaction.hpp:87-184 semantics): when enabled, every shade stage of a pass also
 * keeps a copy of the survivor list it wrote.  read_debug_stage returns, for the LAST pass, the sample ids ("tasks": ((step * pixels + pixel)
 * * 16 + spp)) of the paths that survived `stage` (0 = primary .. 7), in the order of their compacted slots: stable compaction <=> ascending. */
int mvrt_pt_set_debug_capture( mvrt_pt* pt, int enabled );
int mvrt_pt_read_debug_stage( mvrt_pt* pt, int stage, uint32_t* tasksHost, uint64_t capacity, uint32_t* survivorsOut );

/* Counters and timings of the work since the last reset (all steps). */
typedef struct mvrt_pt_stats
{
	uint64_t samples;		 /* paths started */
	uint64_t rays;			 /* intersect() calls (primary + shadow + extra + bounce) */
	uint64_t shadowRays;	 /* of which isShadowRay */
	uint64_t descents;		 /* child fetches of non-shadow rays */
	uint64_t shadowDescents; /* child fetches of shadow rays */
	uint64_t hits;			 /* non-shadow rays that hit */
	uint64_t traceLaunches;	 /* launches of the traversal kernel */
	double traceKernelMs;	 /* summed HIP-event time of the traversal kernel (profiling on) */
	double shadeKernelMs;	 /* summed time of shade+compact kernels (profiling on) */
	double totalKernelMs;	 /* summed time of every kernel of step() (profiling on) */
} mvrt_pt_stats;
/* Failure-path testing: when bytes != 0 the path-state budget of resize / set_pipeline_depth / set_batch_steps is computed against this much "free HBM"
 * instead of what hipMemGetInfo reports.  After a failed (re)allocation the handle has NO frame (steps fail with an error until the next
 * successful mvrt_pt_resize_framebuffer_if_needed). */
int mvrt_pt_set_test_free_bytes( mvrt_pt* pt, uint64_t bytes );
/* Failure-path testing without exhausting the device.  Every device allocation the library makes for itself (not mvrt_malloc) goes through one function.
 * fail_allocation: the nth such allocation from now on THIS thread fails with an error that names this hook, then the hook is off again; 0 turns it off.
 * allocation_state: process-wide tallies -- buffers and bytes held right now, allocations attempted so far; any pointer may be NULL. */
int mvrt_test_fail_allocation( int64_t nth );
int mvrt_test_allocation_state( uint64_t* liveBuffers, uint64_t* liveBytes, uint64_t* totalAllocs );
/* Measuring: *peakOut (may be NULL) = the most bytes the library held at one time, process-wide, since the last reset; reset != 0 starts a new period at what it
 * holds now.  Around one blocking call, peak minus the bytes held before it is the call's scratch plus what it leaves. */
int mvrt_test_peak_bytes( uint64_t* peakOut, int reset );
/* Measuring (tools/ball_bench.py): what the last distance band this thread ran did: out[0..2] = the records of the passes along x, y and z, out[3] = its seeds,
 * out[4] = its cells.  A closing or an opening runs two bands; this is the second. */
int mvrt_test_ball_stats( uint64_t out[5] );
/* Measuring (tools/resample_bench.py): what the last resampling this thread ran did: out[0] = L, the levels of the destination grid, out[l] for l = 1 .. L = the
 * nodes of level l its frontier kept (out[L] = the result cells; 0 from the level on at which nothing was left), the rest 0. */
int mvrt_test_resample_stats( uint64_t out[24] );
/* Measuring (tools/enclosed_nearest_bench.py): what the last mvrt_svo_enclosed_nearest or mvrt_svo_fill_enclosed_nearest of this thread did: out[0] = its enclosed
 * cells, out[1..3] = the gaps of the passes along x, y and z, out[4..6] = the longest gap per axis in cells, out[7] = the deepest d2.  A call that ran no pass
 * (the sizing call, a refusal, zero cells) leaves all but out[0] at 0. */
int mvrt_test_enclosed_nearest_stats( uint64_t out[8] );
/* Measuring (tools/nearest_query_bench.py): what the last mvrt_svo_nearest_voxels, mvrt_svo_nearest_between or mvrt_svo_transfer_attributes of this thread did:
 * out[0] = its queries, out[1] = the node visits in total (non-empty children whose box was tested), out[2] = the most visits of one query, out[3] = the voxels
 * whose distance was taken, the seed's included.  A call that ran no walk (n == 0) leaves all at 0; a refusal made on the host leaves the figures of the call before. */
int mvrt_test_nearest_query_stats( uint64_t out[4] );
int mvrt_pt_set_profiling( mvrt_pt* pt, int enabled ); /* HIP events on `stream` around each kernel of step(); read by get_stats */
int mvrt_pt_reset_stats( mvrt_pt* pt );
int mvrt_pt_get_stats( mvrt_pt* pt, void* stream, mvrt_pt_stats* out ); /* synchronises the stream */

#ifdef __cplusplus
}
#endif
#endif /* MVRT_H */
