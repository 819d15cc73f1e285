// launch.h -- host-side launch wrappers implemented in the .hip translation units.
#pragma once
#include <functional>
#include <utility>

#include "devbuf.h"
#include "mvrt_common.h"

// ---- wavefront path-tracer work buffers (all device pointers, capacity `cap` paths) ---------------
struct PathSet // ping-ponged between shade stages (compacted by the writer)
{
	uint32_t* task;		   // local sample id = ownedPixel * 16 + localSpp
	uint32_t* org;		   // stage k>0: start-below-the-root hint = leading levels of the path of the voxel the ray starts on (traverse_stream.h)
	float *rox, *roy, *roz; // ray origin (stage k>0: the hit point the bounce leaves from)
	float *rdx, *rdy, *rdz; // ray direction (stage k>0: the Lambert bounce direction)
	float *Tx, *Ty, *Tz;	// throughput after the last T *= R
	float *Lx, *Ly, *Lz;	// radiance accumulated so far
	float *nx, *ny, *nz;	// pending next-event contribution, added if the shadow ray misses
};
struct PtBuffers
{
	PathSet set[2];
	float *sx, *sy, *sz; // shadow-ray direction (kind 1), origin = ro
	float *ex, *ey, *ez; // extra Lambert ray direction (kind 2, stage 1 only), origin = ro
	// hit records written by the traversal kernel, one array per ray kind
	float* hitT;	  // kind 0: t (MAX_FLOAT = miss)
	uint8_t* hitN;	  // kind 0: nMajor
	uint8_t* hitS;	  // kind 1: 1 if the shadow ray is occluded
	uint8_t* hitE;	  // kind 2: 1 if the extra ray hit
	uint64_t* hitPath;	// kind 0: voxel path (persistent traversal; vIndex is derived by the shade kernel)
	uint64_t* hitEPath; // kind 2: voxel path
	float *Lsx, *Lsy, *Lsz; // final radiance per sample, indexed by task (read by accumulate)
	uint32_t* blockCount; // survivors per 256-path virtual block; exclusive-scanned in place inside its tile of MVRT_SCAN_TILE blocks (tileBase holds the rest)
	uint32_t* liveCount;  // [stage] number of live paths entering stage k (0..9)
	unsigned long long* cursors; // [16] per-stage ray cursors of the persistent traversal waves (zeroed by generate)
	unsigned long long* stats; // [0] rays [1] shadowRays [2] descents [3] shadowDescents [4] hits [5] samples
	uint64_t cap;
	uint32_t* dbgTasks; // debug capture (host-side use only): [MVRT_MAX_DEPTH][cap] task ids of the survivors each shade stage wrote, in slot order
	const PtBuffers* selfDev; // device-resident copy of this table (read with scalar loads where needed, see PtIO)
	uint32_t* tileBase; // survivors in the scan tiles before each tile (exclusive scan of the tile sums); behind everything else: no older member moves
};
// The survivor scan (kernels_rt.hip): T = MVRT_SCAN_TILE block counts per tile.  A count array for n items holds scanCountEntries( n ) entries and its tile sums
// scanTileEntries( n ): both are padded because the scan loads whole 16-byte quads, and the first is a multiple of 4 so that tile sums carved right behind the
// counts stay 16-byte aligned.
#define MVRT_SCAN_TILE 256
static inline uint64_t scanCountEntries( uint64_t n ) { return ( n / 256 + 8 ) & ~(uint64_t)3; }
static inline uint64_t scanTileEntries( uint64_t n ) { return ( n / 256 + 1 ) / MVRT_SCAN_TILE + 8; }

struct PtFrame
{
	int width, height;
	int tileIndex, tileCount;
	uint64_t ownedPixels;	   // padded to whole 256-pixel blocks
	uint64_t validOwnedPixels; // pixels that exist in the image
	int iteration;			   // iteration of the first step of this batch
	int nSteps;				   // consecutive step() calls merged into this wavefront pass (1..MVRT_MAX_BATCH)
	int traceGridDiv;		   // >1: the traversal launches of this pass take only 1/div of the wave slots (it shares the GPU with a sibling pass)
	int useHints;			   // secondary rays start below the root
};
#define MVRT_MAX_BATCH 8

uint64_t traceWorkspaceLanes();

enum MvrtKernelClass
{
	MVRT_K_TRACE = 0,
	MVRT_K_SHADE = 1,
	MVRT_K_OTHER = 2
};

int launchTraceBatch( const SvoDev& svo, const TraceWorkspace& ws, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz,
					  const uint8_t* isShadow, float* t, int32_t* nMajor, uint32_t* vIndex, uint32_t* descents, hipStream_t stream, const uint64_t* originPath = nullptr );
int launchRenderPrimary( const SvoDev& svo, const TraceWorkspace& ws, const CameraPinhole& cam, int W, int H, int showVertexColor, uchar4* rgba, float* t, int32_t* nMajor, uint32_t* vIndex,
						 uint32_t* descents, hipStream_t stream );
int launchCompactIndices( const uint8_t* keep, uint64_t n, uint32_t* dstIndex, uint32_t* kept, uint32_t* blockScratch, hipStream_t stream );
// the indices i < n with mask[i] != 0, ascending, into list (n entries) and their number into *kept: launchCompactIndices (rankScratch: n entries) and its inverse
int launchActiveList( const uint8_t* mask, uint64_t n, uint32_t* list, uint32_t* kept, uint32_t* rankScratch, uint32_t* blockScratch, hipStream_t stream );

// one PathTracer::step().  `mark(class)` is called before/after each kernel when profiling is on.
struct PtProfiler
{
	virtual void begin( int kernelClass, hipStream_t s ) = 0;
	virtual void end( hipStream_t s ) = 0;
};
// First-hit feature buffers (mvrt_pt_set_aovs).  Kept out of PtBuffers / PtParams on purpose: those are kernel arguments and a device-resident table of the
// traversal and shade kernels, whose offsets must not move.  partA / partN: per (step, pixel) of ONE pass, indexed step * validOwnedPixels + localPixel like Ls*,
// the 16-sample sums { albedo.xyz, hits } and { normal.xyz, t }; albedo / normalDepth: the accumulation buffers, float4 per owned pixel like the frame buffer.
struct AovBuffers
{
	float4 *partA, *partN;
	float4 *albedo, *normalDepth;
};
// active (mvrt_pt_set_sample_mask): the owned pixels this pass samples, ascending, frame.validOwnedPixels of them -- the pass numbers its tasks, Ls* and
// partA / partN over the slots of this list; nullptr = every valid owned pixel, exactly the launches of a library without the mask.  It comes after everything
// else and stays out of PtBuffers / PtParams for the reason given above.
// aov == nullptr: exactly the launches of a library without feature buffers.  moments (mvrt_pt_set_moments; float4 per owned pixel like the frame buffer)
// travels the same way: nullptr = off, no launch
int launchPtStep( const SvoDev& svo, const TraceWorkspace& ws, const HdriDev& hdri, const float2* pmj, const CameraPinhole* cams /* frame.nSteps */, const PtFrame& frame, const PtBuffers& buf, float4* frameBuffer,
				  int numCUs, PtProfiler* prof, hipStream_t stream, hipEvent_t accumulateAfter, const AovBuffers* aov = nullptr, float4* moments = nullptr,
				  const uint32_t* active = nullptr );

// kernels_denoise.hip: the luminance moments of a pass (behind kPtAccumulate, same stream) and the a-trous denoiser on full-frame buffers
int launchPtMoments( const PtBuffers& buf, uint64_t validOwnedPixels, int nSteps, float4* moments, int numCUs, hipStream_t stream, const uint32_t* active = nullptr );
// mask[p] (one byte per owned pixel, padding 0) = 1 where the standard error of the mean luminance exceeds threshold * max( mean, lumFloor ) (mvrt.h,
// mvrt_pt_error_mask); the ones are counted into *countDev (zeroed here).  Not synchronised.
int launchErrorMask( const float4* frameBuffer, const float4* moments, uint64_t validOwnedPixels, uint64_t ownedPixels, float threshold, float lumFloor, int minSamples,
					 int maxSamples, uint8_t* mask, uint32_t* countDev, hipStream_t stream );
uint64_t denoiseScratchBytes( uint64_t nPixels );
struct mvrt_denoise_params; // (mvrt.h)
int launchDenoise( const float4* color, const float4* albedo, const float4* normalDepth, const float4* moments, int W, int H, const mvrt_denoise_params& params, float4* out, void* scratch,
				   hipStream_t stream );

int launchResolve( const float4* fb, uint64_t n, uchar4* out, hipStream_t stream );
int launchAssembleTiles( const float4* gathered, int tileCount, uint64_t rankStridePixels, int W, int H, float4* frame, hipStream_t stream );
// nonEmbedded != 0: psum goes to psumCold (nNodes * 8 u32) and the 8 child masks into Node64::psum[0..1]
int launchConvertNodes( const uint8_t* nodes68, uint32_t nNodes, Node64* out, uint8_t* masks, uint32_t* psumCold, int nonEmbedded, hipStream_t stream );
int launchNodesTo68( const Node64* nodes, const uint8_t* masks, const uint32_t* psumCold, uint32_t nNodes, uint8_t* nodes68, int nonEmbedded, hipStream_t stream );
int launchCheckLeafPsum( const Node64* nodes, const uint8_t* masks, uint32_t nNodes, uint32_t* badDev, hipStream_t stream ); // embedded flavour, after an upload
int launchSplitPsum( Node64* nodes, const uint8_t* masks, uint32_t* psumCold, uint64_t nNodes, hipStream_t stream ); // in place, after a build
// tree flavour -> the reference's 68-byte nodes (mask, children[8], nVoxelsPSum[8]) from { mask, first child } per node
int launchTreeTo68( const uint8_t* masks, const uint32_t* first, const uint32_t* levelBase, const uint32_t* levelCount, int levels, uint32_t nNodes, uint32_t nVoxels, uint8_t* nodes68,
					hipStream_t stream );
int launchCopyKids( const Node64* nodes, uint64_t nNodes, uint32_t* kids, hipStream_t stream ); // embedded flavour: compact children array for the traversal
int launchBuildTopTable( const Node64* nodes, uint32_t rootIndex, uint32_t k, uint2* table, hipStream_t stream ); // embedded flavour only
// embedded flavour: node reference (index | mask << 24) per path prefix of 0..tabLevels levels, level l at prefixTabOffset( l ) (traverse_stream.h)
int launchBuildPrefixRefs( const uint32_t* kids, uint32_t rootRef, uint32_t tabLevels, uint32_t* table, hipStream_t stream );
// cell index of a build (SvoDev::cellBlocks / cellEntries) from its sorted voxel codes: number the occupied blocks (blocks[] preset to ~0, counter to 0), then fill the entries (zeroed)
int launchNumberCellBlocks( const uint64_t* morton, uint64_t n, uint32_t cellBits, uint32_t* blocks, uint32_t* counterDev, hipStream_t stream );
int launchFillCellIndex( const uint64_t* morton, uint64_t n, uint32_t cellBits, const uint32_t* blocks, uint2* entries, hipStream_t stream );
int launchHdriSat( const float4* pixels, int w, int h, double* satF64, uint32_t* satOut, int cosWeighted, f3 axis, double* totalOut, hipStream_t stream );

// GPU SVO construction (svo_build.hip)
// What a build produces, and what an octree handle keeps of it (api_handles.h, Octree).  It owns its arrays: a builder that fails hands nothing over and leaks nothing
struct SvoBuildResult
{
	DevBuf nodes, masks;
	DevBuf psumCold; // non-embedded flavour only
	DevBuf attrs;
	DevBuf morton; // sorted unique codes (an upload has none until mvrt_svo_rebuild)
	uint32_t nNodes = 0, nVoxels = 0, hasEmission = 0;
	uint32_t embedded = 0; // 0 when the octree has >= 0xFFFFFF nodes (IntersectorOctreeGPU.hpp:231) or on request
	uint64_t totalDumped = 0;
	// "tree" flavour (no DAG, masks not embedded): `nodes` holds nBricks two-level bricks, `masks` the per-node masks and `treeFirst` the
	// per-node first-child index (reference numbering); node ranges per builder level (0 = parents of voxels)
	uint32_t tree = 0, nBricks = 0, treeRoot = 0;
	DevBuf treeFirst;
	uint32_t treeLevelBase[24] = { 0 }, treeLevelCount[24] = { 0 };
};
static inline int levelsOf( int gridRes ) // log2 of a power of two, -1 for anything else (zero, negative, not a power of two): every int terminates
{
	if( gridRes <= 0 || ( gridRes & ( gridRes - 1 ) ) != 0 ) return -1;
	int l = 0;
	while( ( gridRes >> l ) != 1 ) l++;
	return l;
}
// flags: 1 = no DAG de-duplication (every sibling group is a node), 2 = never embed masks in child pointers
int svoBuildFromTriangles( const float* vertsHost, const float* colsHost, const float* emisHost, uint64_t nVertices, f3 origin, float dps, int gridRes, int flags,
						   hipStream_t stream, SvoBuildResult* out );
int svoBuildSynthetic( uint64_t nRandomVoxels, uint64_t seed, int gridRes, int flags, hipStream_t stream, SvoBuildResult* out );
// voxel lists (device arrays): xyz = 3 x u32 per entry, attribs = VoxelAttirb (8 bytes) per entry or NULL (white, no emission)
int svoBuildFromVoxels( const uint32_t* xyz, const uint32_t* attribs, uint64_t n, int gridRes, int flags, hipStream_t stream, SvoBuildResult* out );
// a batch of edits (ops: 0 remove, 1 set; NULL = all set; last entry per voxel wins) against the sorted unique list of a build.  *structural = 1: out holds the
// new octree (the old arrays are untouched); 0: the attributes were changed in place (node structure unchanged), *hasEmissionOut = the new flag
int svoEditVoxels( const uint64_t* oldMorton, uint2* oldAttrs, uint32_t nOld, const uint32_t* xyz, const uint32_t* attribs, const uint8_t* ops, uint64_t n, int gridRes, int flags,
				   hipStream_t stream, SvoBuildResult* out, int* structural, uint32_t* hasEmissionOut );
// the levels over n sorted unique codes and their attributes (both handed to *out on success), as svoBuildFromVoxels builds them behind its sort: the attribute
// bytes are kept verbatim and out->hasEmission is 0 -- the caller knows the flag of the set it hands in (mvrt_svo_rebuild)
int svoBuildFromSorted( DevBuf& morton, DevBuf& attrs, uint32_t n, int gridRes, int flags, hipStream_t stream, SvoBuildResult* out );

// surface extraction (kernels_surface.hip; mvrt_svo_surface_masks / _quads / _mesh): what it reads of a built octree.  cellBlocks == nullptr: no cell index,
// neighbours are searched in the codes.  The calls block (the counts go back to the host), keep their scratch in DevBufs and write NOTHING to the caller's
// arrays unless they succeed.
struct SurfaceSource
{
	const uint64_t* morton; // sorted unique voxel codes
	uint32_t nVoxels, levels;
	const uint32_t* cellBlocks;
	const uint2* cellEntries;
	uint32_t cellBits;
	f3 lower;
	float dps;
	const uint2* attrs; // VoxelAttirb per voxel, read by surfaceMerged only
};
int surfaceMasks( const SurfaceSource& s, uint8_t* masksDev, uint64_t* nFacesOut, hipStream_t stream );
// the masks kernel alone (masks == nullptr: count only); the sum of the popcounts is added to *nFacesDev.  Not synchronised.
int launchSurfaceMasks( const SurfaceSource& s, uint8_t* masks, unsigned long long* nFacesDev, hipStream_t stream );
// givenMasks (the _masked calls; nullptr = the exposure masks): nVoxels bytes whose set bits 0..5 are the faces, taken as given; the error messages name the _masked call
int surfaceQuads( const SurfaceSource& s, const uint8_t* givenMasks, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, uint64_t* nFacesOut,
				  hipStream_t stream );
int surfaceMesh( const SurfaceSource& s, const uint8_t* givenMasks, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev,
				 float* verticesDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, hipStream_t stream );
// flags: MVRT_SURFACE_MERGE_* (mvrt.h), checked by the caller, as is that indicesDev / verticesDev come with the weld flag only
int surfaceMerged( const SurfaceSource& s, const uint8_t* givenMasks, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev, uint8_t* rectDirDev,
				   uint32_t* rectSizeDev, float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFacesOut, uint64_t* nRectsOut, uint64_t* nVerticesOut,
				   hipStream_t stream );
// constrained surface nets on the welded mesh (kernels_smooth.hip; mvrt_svo_surface_smooth): the mesh of surfaceMesh with relaxed vertex positions.  The rule's
// ranges are checked by the caller; the sizing call runs no iteration
struct SmoothRule
{
	int32_t iterations, weightEven, weightOdd, limit;
};
int surfaceSmooth( const SurfaceSource& s, const uint8_t* givenMasks, const SmoothRule& rule, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev,
				   uint32_t* indicesDev, float* verticesDev, int32_t* displacementsDev, uint8_t* neighboursDev, uint64_t* nFacesOut, uint64_t* nVerticesOut, uint64_t* clampedOut,
				   hipStream_t stream );

// enclosed empty cells (kernels_fill.hip; mvrt_svo_enclosed_cells / mvrt_svo_fill_enclosed): only morton, nVoxels and levels of the source are read.  The calls
// block, keep their scratch in DevBufs and write NOTHING to the caller's arrays unless they succeed.
int enclosedCells( const SurfaceSource& s, uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint64_t* nCellsOut, uint64_t* nRegionsOut, hipStream_t stream );
// the same cells in no particular order into xyz (allocated here, 3 x u32 per cell; left empty when there are none or 2^32 or more: the caller looks at *nCells)
int enclosedCellsUnordered( const SurfaceSource& s, DevBuf& xyz, uint64_t* nCells, hipStream_t stream );
// exterior masks (mvrt_svo_surface_exterior_masks): the exposure masks with the bits that look into an enclosed cell cleared, from the front half of the
// classification above (linear keys, unions, flatten) and the masks kernel of kernels_surface.hip.  masksDev == nullptr: counts only
int surfaceExteriorMasks( const SurfaceSource& s, uint8_t* masksDev, uint64_t* nFacesOut, uint64_t* nHiddenOut, hipStream_t stream );
int launchFillAttribs( uint2 attrib, uint64_t n, uint2* out, hipStream_t stream ); // n copies of one VoxelAttirb.  Not synchronised.
// What the classification of kernels_fill.hip leaves: the sorted linear keys ( z << 2L | y << L | x ) of the voxels, the flattened roots (node i + 1 = gap i, the
// empty run between sorted voxels i and i + 1 of one row; root 0 = EXTERIOR) and the n + 1 exclusive cell offsets of the enclosed gaps.  The counts are valid
// when enclosedClassify returns
struct EnclosedClassified
{
	DevBuf count, lin, root, offs;
	uint64_t nCells = 0, nRegions = 0;
};
int enclosedClassify( const SurfaceSource& s, EnclosedClassified* out, hipStream_t stream );
// roots: the root of every cell of a listing in ascending Morton code.  firstCell (nVoxels + 1 entries, allocated here) = per root the position of its first cell,
// rank1 (allocated here) = the inclusive count of first cells: the region of cell c is rank1[firstCell[roots[c]]] - 1.  Waits for the stream
int enclosedRegionRanks( const uint32_t* roots, uint32_t nCells, uint32_t nVoxels, DevBuf& firstCell, DevBuf& rank1, hipStream_t stream );

// nearest voxel of the enclosed cells (kernels_nearest.hip; mvrt_svo_enclosed_nearest / mvrt_svo_fill_enclosed_nearest): morton, attrs, nVoxels and levels of the
// source are read.  The calls block, keep their scratch in DevBufs and write NOTHING to the caller's arrays unless they succeed.
struct NearestStats // what the last call of this thread did (tools/enclosed_nearest_bench.py through mvrt_test_enclosed_nearest_stats)
{
	uint64_t cells = 0, gaps[3] = { 0, 0, 0 }, longest[3] = { 0, 0, 0 }, deepest = 0; // per axis x, y, z; all but cells stay 0 where no pass was run
};
int enclosedNearest( const SurfaceSource& s, uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev,
					 uint64_t* nCellsOut, uint64_t* nRegionsOut, hipStream_t stream );
// the same cells in no particular order with the attribute of their nearest voxel, for the edit (xyz 3 x u32, attribs 8 bytes per cell, allocated here; left empty
// when there are no cells or nVoxels + *nCells >= 2^32 - 1: the caller looks at *nCells)
int enclosedNearestUnordered( const SurfaceSource& s, DevBuf& xyz, DevBuf& attribs, uint64_t* nCells, hipStream_t stream );
NearestStats nearestLastStats(); // of this thread

// nearest voxel of arbitrary lattice points (kernels_query.hip; mvrt_svo_nearest_voxels / mvrt_svo_nearest_between / mvrt_svo_transfer_attributes): morton, attrs,
// nVoxels and levels of the sources are read; the query range, the offset, the flags and n < 2^32 are checked by the caller.  The calls block, keep their scratch in
// DevBufs and write NOTHING to the caller's arrays before their last allocation and check have passed.
struct NearestQueryStats // what the last call of this thread did (tools/nearest_query_bench.py through mvrt_test_nearest_query_stats)
{
	uint64_t queries = 0, visits = 0, mostVisits = 0, compared = 0;
};
struct NearestBetweenCounts
{
	uint64_t n = 0, maxDist2 = 0, nZero = 0, nBeyond = 0;
	uint32_t farthest = 0;
};
int nearestVoxels( const SurfaceSource& s, uint64_t n, const int32_t* queryDev, uint64_t maxDist2, uint64_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, hipStream_t stream );
// every voxel of a, moved by -o, queried in b
int nearestBetween( const SurfaceSource& a, const SurfaceSource& b, const int32_t o[3], uint64_t maxDist2, uint64_t capacity, uint64_t* dist2Dev, uint32_t* nearestDev,
					NearestBetweenCounts* counts, hipStream_t stream );
// the list the attribute-only edit takes: the voxels of dst with a nearest voxel of src within the limit (*nTaken of them, xyz 3 x u32 and attribs 8 bytes, allocated
// here) with the bytes they end with.  *nChanged == 0: no byte would change and no list is made
int nearestTransferList( const SurfaceSource& dst, const SurfaceSource& src, const int32_t o[3], uint64_t maxDist2, uint32_t flags, DevBuf& xyz, DevBuf& attribs, uint64_t* nTaken,
						 uint64_t* nChanged, uint64_t* nBeyond, hipStream_t stream );
NearestQueryStats nearestQueryLastStats(); // of this thread

// ---- sorted voxel lists (kernels_list.hip) -------------------------------------------------------------------------------------------------------------
// What every voxel-set operator hands to svoBuildFromSorted: n sorted unique codes with their attributes and the emission flag over them, allocated by the
// operator.  The one convention of "nothing changed": the arrays are left empty and n is the voxel count of the set the operator started from.
struct SortedVoxels
{
	DevBuf codes, attrs;
	uint32_t n = 0, hasEmission = 0;
	bool unchanged( uint32_t nVoxels ) const { return !codes.p && !attrs.p && n == nVoxels; }
};
// the list a sequence of steps works on: borrowed arrays first (the handle's, not owned), then the arrays the last step made
struct VoxelList
{
	const uint64_t* codes;
	const uint2* attrs;
	uint32_t n;
	DevBuf ownCodes, ownAttrs;
	VoxelList( const uint64_t* c, const uint2* a, uint32_t count ) : codes( c ), attrs( a ), n( count ) {}
	void take( DevBuf& c, DevBuf& a, uint32_t count )
	{
		ownCodes = std::move( c );
		ownAttrs = std::move( a );
		codes = ownCodes.as<uint64_t>();
		attrs = ownAttrs.as<uint2>();
		n = count;
	}
};
// The list steps; each allocates its outputs itself and has waited for the stream when it returns.  Two sorted lists without a common code merged into one; the
// attributes that the n codes, a subset of srcCodes, have there; *hasEmission = 1 where one of the n attributes has an emission byte set
int mergeLists( const uint64_t* aCodes, const uint2* aAttrs, uint32_t nA, const uint64_t* bCodes, const uint2* bAttrs, uint32_t nB, DevBuf& codes, DevBuf& attribs, hipStream_t stream );
int gatherAttrs( const uint64_t* codes, uint32_t n, const uint64_t* srcCodes, const uint2* srcAttrs, uint32_t nSrc, DevBuf& attribs, hipStream_t stream );
int anyEmission( const uint2* attrs, uint32_t n, uint32_t* hasEmission, hipStream_t stream );
// offs = the n + 1 exclusive sums of the flags ( mask[i] != 0 ) == ( removed != 0 ), *count = their number; then the flagged entries in order: code and attribute
// (a step) or index (a listing), any output may be null.  The launch is not synchronised.  maskOffsets with removed = 1 is the scan of every compaction by a
// 32-bit flag array: the erosion listing, the seeds, the cells outside the set and the shallow voxels of the round offsets (kernels_ball.hip)
int maskOffsets( const uint32_t* mask, uint32_t n, uint32_t removed, DevBuf& offs, uint32_t* count, hipStream_t stream );
int launchCompactMasked( const uint64_t* codes, const uint2* attrs, const uint32_t* mask, const uint32_t* offs, uint32_t n, uint32_t removed, uint64_t* codesOut, uint2* attrsOut,
						 uint32_t* vIndexOut, hipStream_t stream );
// the erosion's scan and scatter on a caller's mask: the entries of the n sorted codes and attributes whose mask is 0, in order (out.n of them; the arrays are
// left empty when that is 0 or n), and with scanEmission the emission flag over them
int compactUnmasked( const uint64_t* srcCodes, const uint2* srcAttrs, const uint32_t* mask, uint32_t n, bool scanEmission, SortedVoxels& out, hipStream_t stream );
// One dilate / erode / close / open on the list of s: the halves in the order of the operator, the unchanged test by the count, the opening's re-gather of the
// original attribute bytes, the emission scan and the move into `out`.  A half returns non-zero on failure and leaves the list alone when it changes nothing.
// idleFirstHalfEnds: a first half that changes nothing ends the call (the second is not run)
enum
{
	MVRT_MORPH_OP_DILATE = 0,
	MVRT_MORPH_OP_ERODE = 1,
	MVRT_MORPH_OP_CLOSE = 2,
	MVRT_MORPH_OP_OPEN = 3
};
typedef std::function<int( VoxelList& )> ListHalf;
int runListOperator( int op, const SurfaceSource& s, bool idleFirstHalfEnds, const ListHalf& dilate, const ListHalf& erode, SortedVoxels& out, hipStream_t stream );
// The tail of a listing call, behind its counts: the sizing call is done, a capacity below n is refused ("<who>: <capacityName> <capacity> is smaller than the
// <n> <things>; nothing was written", listingRefusal), an empty listing is done, else the caller writes its arrays
enum
{
	LISTING_DONE = 0,
	LISTING_REFUSED = 1,
	LISTING_WRITE = 2
};
int listingTail( const char* who, const char* capacityName, const char* things, bool sizing, uint64_t capacity, uint64_t n );
void listingRefusal( const char* who, const char* capacityName, const char* things, uint64_t capacity, uint64_t n );

// affine resampling (kernels_resample.hip; mvrt_svo_resample_voxels / mvrt_svo_resample): morton, attrs, nVoxels and levels of the source are read; m[9] and t[3] are
// the inverse map of mvrt_cell_transform, within its limits (resampleTransformValid), and dstLevels = log2 of the destination gridRes in [1, 21], all checked by the
// caller.  The calls block, keep their scratch in DevBufs and write NOTHING to the caller's arrays unless they succeed.  A frontier or a result of 2^32 - 1 entries
// or more is refused; `who` names the call
struct ResampleStats // what the last refinement of this thread did (tools/resample_bench.py through mvrt_test_resample_stats)
{
	uint32_t levels = 0;	 // of the destination grid
	uint64_t frontier[22] = {}; // frontier[l], l = 1 .. levels: the surviving nodes of level l; frontier[levels] = the result cells
};
bool resampleTransformValid( const int64_t m[9], const int64_t t[3] );
int resampleVoxels( const SurfaceSource& s, const int64_t m[9], const int64_t t[3], uint32_t dstLevels, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* sourceDev,
					uint64_t* nOut, hipStream_t stream );
// the same list as sorted codes and attributes for svoBuildFromSorted (left empty when the result is: the caller looks at out.n)
int resampleList( const char* who, const SurfaceSource& s, const int64_t m[9], const int64_t t[3], uint32_t dstLevels, SortedVoxels& out, hipStream_t stream );
ResampleStats resampleLastStats(); // of this thread

// coarse cells (kernels_coarsen.hip; mvrt_svo_coarse_voxels / mvrt_svo_coarsen): the n >= 1 sorted codes and Morton-ordered attributes of a build, levelsDown in
// [1, levels - 1] and minCount in [1, coarseCellCapacity( levelsDown )], all checked by the caller.  The calls block, keep their scratch in DevBufs and write
// NOTHING to the caller's arrays unless they succeed.
uint64_t coarseCellCapacity( int levelsDown ); // 8^levelsDown, the fine voxels one coarse cell can hold (levelsDown <= 20)
int coarseVoxels( const uint64_t* morton, const uint2* attrs, uint32_t n, int levelsDown, uint64_t minCount, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev,
				  uint32_t* countDev, uint64_t* nOut, hipStream_t stream );
// the same list as sorted codes and attributes for svoBuildFromSorted (left empty when no cell is kept: the caller looks at out.n)
int coarseList( const uint64_t* morton, const uint2* attrs, uint32_t n, int levelsDown, uint64_t minCount, SortedVoxels& out, hipStream_t stream );
// every cell of the listing with minCount = 1 as device arrays allocated here, in its order: ascending codes, attributes and voxel counts (*nCells >= 1 of each).
// On failure the three arrays are left as they were
int coarseCells( const uint64_t* morton, const uint2* attrs, uint32_t n, int levelsDown, DevBuf& codes, DevBuf& attribs, DevBuf& counts, uint32_t* nCells, hipStream_t stream );

// dilation, erosion, closing and opening (kernels_morph.hip; mvrt_svo_dilation_cells / _erosion_voxels / _dilate / _erode / _close / _open): morton, attrs, nVoxels
// and levels of the source are read, element is MVRT_MORPH_FACES or MVRT_MORPH_CUBE, checked by the caller.  The calls block, keep their scratch in DevBufs and
// write NOTHING to the caller's arrays unless they succeed.
int morphDilationCells( const SurfaceSource& s, int element, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* countDev, uint64_t* nOut, hipStream_t stream );
int morphErosionVoxels( const SurfaceSource& s, int element, uint64_t capacity, uint32_t* vIndexDev, uint64_t* nOut, hipStream_t stream );
// the cells one dilation step adds to the n sorted codes, as ascending codes into cellCodes (allocated here; left empty when *nCells is 0: a full grid).  Blocks
int morphStepCodes( const char* who, const uint64_t* codes, const uint2* attrs, uint32_t n, uint32_t levels, int element, DevBuf& cellCodes, uint32_t* nCells, hipStream_t stream );
// `steps` >= 1 steps of the operator (MVRT_MORPH_OP_*) on sorted lists.  A step that would reach 2^32 - 1 voxels or leave none is refused; `who` names the call
int morphList( const char* who, const SurfaceSource& s, int element, int op, int steps, SortedVoxels& out, hipStream_t stream );

// round offsets (kernels_ball.hip; mvrt_svo_distance_cells / _depth_voxels / _dilate_ball / _erode_ball / _close_ball / _open_ball): morton, attrs, nVoxels and levels
// of the source are read, radius2 is in [1, 1024], checked by the caller.  The calls block, keep their scratch in DevBufs and write NOTHING to the caller's arrays
// unless they succeed.
struct BallStats // what the last band of a call did (tools/ball_bench.py through mvrt_test_ball_stats)
{
	uint64_t records[3] = { 0, 0, 0 }; // per pass x, y, z
	uint64_t seeds = 0, cells = 0;
};
int ballDistanceCells( const SurfaceSource& s, uint32_t radius2, uint64_t capacity, uint32_t* xyzDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, uint64_t* nOut,
					   hipStream_t stream );
int ballDepthVoxels( const SurfaceSource& s, uint32_t radius2, uint64_t capacity, uint32_t* vIndexDev, uint32_t* depth2Dev, uint64_t* nOut, hipStream_t stream );
// the operator (MVRT_MORPH_OP_*) with the ball of radius2 on sorted lists.  A result of 2^32 - 1 voxels or more or of none is refused; `who` names the call
int ballList( const char* who, const SurfaceSource& s, uint32_t radius2, int op, SortedVoxels& out, hipStream_t stream );
BallStats ballLastStats(); // of this thread

// connected components (kernels_components.hip; mvrt_svo_components / mvrt_svo_keep_components): morton, attrs, nVoxels and levels of the source are read, element
// is MVRT_MORPH_FACES or MVRT_MORPH_CUBE, checked by the caller.  The calls block, keep their scratch in DevBufs and write NOTHING to the caller's arrays
// unless they succeed.
int componentsList( const SurfaceSource& s, int element, uint32_t* labelDev, uint64_t capacity, uint32_t* sizeDev, uint32_t* firstDev, uint32_t* boxDev, uint64_t* nComponentsOut,
					uint64_t* largestOut, hipStream_t stream );
// the voxels of the kept components (minVoxels >= 1, checked by the caller) as a sorted list: unchanged when every component is kept, out.n == 0 when none is
// (the caller refuses)
int componentsKeepList( const SurfaceSource& s, int element, uint64_t minVoxels, uint32_t keepLargest, SortedVoxels& out, uint32_t* nComponents, uint32_t* nKeptComponents,
						hipStream_t stream );

// two voxel sets (kernels_combine.hip; mvrt_svo_combine_voxels / mvrt_svo_combine): morton, attrs, nVoxels and levels of a, morton, attrs and nVoxels of b (its
// levels only decide whether its codes can stand as they are), op and flags as in mvrt.h and o[3] in [-2^21, 2^21], all checked by the caller.  The calls block,
// keep their scratch in DevBufs and write NOTHING to the caller's arrays unless they succeed.
enum
{
	MVRT_COMBINE_OP_UNION = 0,
	MVRT_COMBINE_OP_INTERSECTION = 1,
	MVRT_COMBINE_OP_DIFFERENCE = 2,
	MVRT_COMBINE_OP_XOR = 3,
	MVRT_COMBINE_FLAG_ATTRIB_B = 1
};
int combineVoxels( const SurfaceSource& a, const SurfaceSource& b, int op, const int32_t o[3], uint32_t flags, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev,
				   uint8_t* sourceDev, uint64_t* nOut, uint64_t* nOverlapOut, uint64_t* nClippedOut, hipStream_t stream );
struct CombineCounts
{
	SortedVoxels list;						 // the result.  nAdded == nRemoved == 0: with recolours only list.attrs is filled (the codes are a's), without it nothing is
	uint64_t nOverlap = 0, nClipped = 0;	 // A n B', the entries of b the offset moves out of the grid
	uint32_t nAdded = 0, nRemoved = 0;		 // B' \ A where the operator takes it, the voxels of A it drops
	uint32_t recolours = 0;					 // the overlap survives and takes b's attributes
};
// A result of no voxel or of 2^32 - 1 or more is refused; `who` names the call
int combineList( const char* who, const SurfaceSource& a, const SurfaceSource& b, int op, const int32_t o[3], uint32_t flags, CombineCounts* counts, hipStream_t stream );

// octree walk (kernels_walk.hip;mvrt_svo_walk_voxels / mvrt_svo_rebuild): what it reads of an embedded or plain octree, built or uploaded (never the tree
// flavour, which always keeps its codes).  The calls block, keep their scratch in DevBufs and never write to the octree.
struct WalkSource
{
	const Node64* nodes;
	const uint8_t* masks;	  // per-node own mask (read in the plain flavour)
	const uint32_t* psumCold; // plain flavour: nVoxelsPSum[node * 8 + child]
	uint32_t nNodes, levels, embedded, rootMask;
};
struct WalkResult
{
	DevBuf codes, vIndex; // per path, ascending: the Morton code (uint64) and the nVoxelsPSum sum (uint32)
	uint64_t n = 0;		  // paths, whether or not the arrays were filled
	int filled = 0;
};
// counts the root-to-voxel paths; fill && n <= fillLimit: also lists them (n == 0: nothing to list, filled stays 0)
int walkPaths( const WalkSource& s, bool fill, uint64_t fillLimit, WalkResult* out, hipStream_t stream );
// per entry i < n: xyz = the decoded code, vIndexOut = v, attribs = attrs[v] with v = vIndex[i] (vIndex == nullptr: v = i); any output may be null.  Not synchronised.
int launchWalkGather( const uint64_t* codes, const uint32_t* vIndex, const uint2* attrs, uint32_t nVoxels, uint64_t n, uint32_t* xyz, uint32_t* vIndexOut, uint32_t* attribs,
					  hipStream_t stream );
// mvrt_svo_read_voxels: the same kernel on the sorted list of a build (entry i = voxel i).  Waits for the stream.
int svoReadVoxels( const uint64_t* morton, const uint2* attrs, uint32_t n, uint32_t* xyz, uint32_t* attribs, hipStream_t stream );

// distance-limited rays and the ambient occlusion bake (kernels_range.hip; mvrt_trace_batch_range / mvrt_ao_directions / mvrt_svo_surface_ao): the per-lane walk of
// include/mvrt/device.hpp on the view mvrt_svo_device_view fills.  launchTraceRange is asynchronous; surfaceAo validates the entries on the device, blocks, keeps
// its scratch in one DevBuf and writes NOTHING to `open` unless every entry is in range.
struct mvrt_device_octree;
int launchTraceRange( const mvrt_device_octree& view, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz,
					  const uint8_t* isShadow, const float* tMax, float* t, int32_t* nMajor, uint32_t* vIndex, uint32_t* descents, hipStream_t stream );
// level of detail per ray (kernels_lod.hip; mvrt_svo_lod_prepare / mvrt_trace_batch_cone / mvrt_render_primary_lod): the attribute pyramid of a built octree and
// the cone walk of include/mvrt/device.hpp (DeviceOctree::intersectConeEx, DeviceLod) on the views mvrt_svo_device_view and mvrt_svo_lod_view fill.
// Entry L of the pyramid = level L in [1, levels - 1]: what coarseCells lists with levelsDown = levels - L.  It owns its arrays; an octree handle keeps one
// (api_handles.h, Octree) so that whatever replaces or clears the octree drops it
struct LodPyramid
{
	DevBuf codes[16], attrs[16], counts[16];
	uint32_t n[16] = { 0 };
	uint32_t ready = 0;
	uint64_t bytes() const
	{
		uint64_t b = 0;
		for( int l = 0; l < 16; l++ ) b += codes[l].bytes + attrs[l].bytes + counts[l].bytes;
		return b;
	}
};
// builds every level from the n sorted codes and attributes of a build with levels in [1, 16]; blocks.  On failure *out is left empty
int lodBuild( const uint64_t* morton, const uint2* attrs, uint32_t n, uint32_t levels, LodPyramid* out, hipStream_t stream );
struct mvrt_device_lod;
// lod == nullptr: index and attrib are null too.  Asynchronous
int launchTraceCone( const mvrt_device_octree& view, const mvrt_device_lod* lod, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy,
					 const float* rdz, const float* coneA, const float* coneB, float* t, int32_t* nMajor, uint32_t* level, uint64_t* cellCode, uint32_t* index, uint32_t* attrib,
					 uint32_t* descents, hipStream_t stream );
// lod == nullptr: the hit normal is the colour.  Asynchronous
int launchRenderLod( const mvrt_device_octree& view, const mvrt_device_lod* lod, const float camera[15], int W, int H, float coneB, uchar4* rgba, float* t, int32_t* nMajor,
					 uint32_t* level, uint32_t* descents, hipStream_t stream );
bool aoSamplesOk( int samples );				// a power of two in [1, 256]
void aoDirections( int samples, float* dirs ); // host only: 6 * samples * 3 floats
int surfaceAo( const mvrt_device_octree& view, const uint64_t* morton, uint64_t nFaces, const uint32_t* faceVoxel, const uint8_t* faceDir, int samples, float radius,
			   uint16_t* open, hipStream_t stream );
