// api_handles.h -- what the parts of the C-ABI share: api.hip (runtime, octree handles, batch traces), api_voxels.hip (the voxel-set operators) and
// api_pt.hip (the path tracer, which meets the others in the octree handle alone).  Host code only.
#pragma once
#include <string.h>

#include <utility>

#include "../../include/mvrt.h"
#include "launch.h"

#define MVRT_EXPORT extern "C" __attribute__( ( visibility( "default" ) ) )

#define REQUIRE( cond, ... )          \
	do                                \
	{                                 \
		if( !( cond ) )               \
		{                             \
			mvrtSetError( __VA_ARGS__ ); \
			return 1;                 \
		}                             \
	} while( 0 )

// the refusal of build flags other than the two a voxel-list build knows, in the name of the call `who`
#define REQUIRE_BUILD_FLAGS( who, flags ) \
	REQUIRE( ( ( flags ) & ~( MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK ) ) == 0, "%s: unsupported flags 0x%x (MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK only)", who, flags )

// scratch of the persistent traversal kernels with its owner: one per octree handle and one per pipeline slot of a path tracer
struct Workspace
{
	DevBuf wsBuf, pathBuf; // spill rows + cursor, sized on demand; per-ray paths
	TraceWorkspace ws = { nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr };
	int ensure( uint32_t levels, uint64_t nPaths )
	{
		if( nPaths > ws.pathCap )
		{
			ws.paths = nullptr;
			ws.pathCap = 0;
			if( pathBuf.alloc( nPaths * 12 ) ) return 1; // 8-byte path + 4-byte t scratch per ray
			ws.paths = pathBuf.as<uint64_t>();
			ws.pathCap = nPaths;
		}
		const uint64_t lanes = traceWorkspaceLanes();
		const uint64_t rows = 2 * (uint64_t)( levels ? levels : 1 ) + 2; // fast path: 1 row per level; irregular rays: 2 per slot
		const uint64_t bytes = 256 + rows * lanes * ( sizeof( uint4 ) + 2 * sizeof( uint32_t ) );
		if( wsBuf.bytes < bytes && wsBuf.alloc( bytes ) ) return 1;
		ws.cursor = (unsigned long long*)wsBuf.p;
		ws.spill = (uint4*)( (uint8_t*)wsBuf.p + 256 );
		ws.spillStride = lanes;
		ws.spillMask = (uint32_t*)( ws.spill + rows * lanes );
		ws.spillMask2 = ws.spillMask + rows * lanes;
		return 0;
	}
};

// ---- IntersectorOctreeGPU -------------------------------------------------------------------------------
// Everything that describes one resident octree.  The calls that make one fill a local Octree and move it into the handle when it is complete, derived
// tables included: a handle holds a whole octree or an empty one (numberOfNodes == 0), which every entry point that reads an octree refuses on the host.
// The main arrays, the counts and the tree description are the builder's record (launch.h), taken over whole from a build and filled in by an upload; what
// is derived from them lives here.
struct Octree : SvoBuildResult
{
	Octree() {}
	explicit Octree( SvoBuildResult&& built ) : SvoBuildResult( std::move( built ) ) {}
	DevBuf kids;	 // embedded flavour: children[8] per node, 32 B per node (what the traversal reads)
	DevBuf topTable; // per-prefix start of the nVoxelsPSum walk (SvoDev::topTable), embedded flavour
	uint32_t topLevels = 0;
	DevBuf cellBlocks, cellEntries; // SvoDev::cellBlocks / cellEntries, only after build()
	uint32_t cellBits = 0;
	mvrt_svo_info info = {}; // bounds, dps, gridRes, levels: the counts are the record's and emissionScale the handle's (mvrt_svo_get_info)
	uint8_t rootMask = 0;
	uint32_t leafPsumIsPopcount = 1; // (uploads: checked, see launchCheckLeafPsum)
	int buildFlags = 0;				 // MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK of the build, kept by edits
	// the attribute pyramid (mvrt_svo_lod_prepare): part of the octree record, so whatever replaces or clears the octree drops it; an edit that rewrites
	// the attributes in place drops it by hand (editHandle)
	LodPyramid lod;
};
struct mvrt_svo
{
	Octree oct;
	mutable Workspace work;		 // one per handle; users of one handle must be stream-ordered
	float emissionScale = 7.5f; // IntersectorOctreeGPU.hpp:273
	mvrt_pt* owner = nullptr;	 // the PathTracer this is the m_intersectorOctreeGPU of (its deferred / in-flight steps read this octree)
	bool empty() const { return oct.nNodes == 0; }
	void cleanUp() { oct = Octree(); } // :26-38
	int ensureWorkspace( uint64_t nPaths = 0 ) const { return work.ensure( oct.info.levels, nPaths ); }
	SvoDev dev() const
	{
		const mvrt_svo_info& info = oct.info;
		SvoDev d;
		d.nodes = oct.nodes.as<Node64>();
		d.masks = oct.masks.as<uint8_t>();
		d.psumCold = oct.psumCold.as<uint32_t>();
		d.attrs = oct.attrs.as<uint2>();
		d.nNodes = oct.nNodes;
		d.nVoxels = oct.nVoxels;
		d.lower = mk3( info.lower[0], info.lower[1], info.lower[2] );
		d.upper = mk3( info.upper[0], info.upper[1], info.upper[2] );
		d.dps = info.dps;
		d.emissionScale = emissionScale;
		d.hasEmission = oct.hasEmission;
		d.embedded = oct.embedded;
		d.levels = info.levels;
		d.rootIndex = oct.nNodes - 1; // root = last node, :250
		d.rootMask = oct.rootMask;
		d.kids = oct.kids.as<uint32_t>();
		d.topTable = oct.topTable.as<uint2>();
		d.topLevels = oct.topLevels;
		d.cellBlocks = oct.cellEntries.p ? oct.cellBlocks.as<uint32_t>() : nullptr;
		d.cellEntries = oct.cellEntries.as<uint2>();
		d.cellBits = oct.cellBits;
		d.tree = oct.tree;
		d.treeRoot = oct.treeRoot;
		d.leafPsumIsPopcount = oct.leafPsumIsPopcount;
		return d;
	}
};

static inline CameraPinhole cameraFrom15( const float c[15] ) // the 15 floats of the ABI (mvrt.h) are the struct's
{
	CameraPinhole cam;
	memcpy( &cam, c, sizeof( cam ) );
	return cam;
}

// The reference's step() passes m_intersectorOctreeGPU and m_hdri to the kernel BY VALUE at call time (PathTracer.hpp:150-169).  step() is
// deferred here, so every change of state a pending or in-flight step reads is preceded by launching (flush) or finishing (drain) those steps.
int ptFlush( mvrt_pt* pt ); // (api_pt.hip)
int ptDrain( mvrt_pt* pt );

// What api.hip and api_voxels.hip share.  ownerDrain finishes the steps of the path tracer that owns the handle; adoptBuild, adoptOnOwnGrid, adoptSortedOnGrid and
// adoptSorted are the only ways a handle takes a new octree and editHandle is the only way it is edited from a device list (api.hip, where each says what a failure
// leaves); surfaceSource refuses a handle without sorted codes, in the name of the call `who`, and fills what the passes read (api_voxels.hip)
int ownerDrain( const mvrt_svo* svo );
int adoptBuild( mvrt_svo* svo, SvoBuildResult& r, const float origin[3], float dps, int gridRes, int flags );
int adoptOnOwnGrid( mvrt_svo* svo, SvoBuildResult& r, int flags );
int adoptSortedOnGrid( mvrt_svo* svo, SortedVoxels& v, uint64_t totalDumped, const float origin[3], float dps, int gridRes, int flags, uint64_t* nOut, hipStream_t stream );
int adoptSorted( mvrt_svo* svo, SortedVoxels& v, hipStream_t stream );
enum // the outcomes of an edit that a caller of editHandle accepts
{
	EDIT_STRUCTURAL = 1,
	EDIT_ATTRIBUTES = 2
};
int editHandle( mvrt_svo* svo, const char* who, int accepts, const uint32_t* xyz, const uint32_t* attribs, const uint8_t* ops, uint64_t n, DevBuf* ownXyz, DevBuf* ownAttribs,
				hipStream_t stream );
int surfaceSource( const mvrt_svo* svo, const char* who, SurfaceSource* s );
