// api.hip -- the C-ABI of libmvrt_hip.so (include/mvrt.h), first half: the runtime pass-throughs, the octree handle (the reference's host struct
// IntersectorOctreeGPU, IntersectorOctreeGPU.hpp:21-275, behind an opaque handle), the batch traces and the camera.  The path tracer is api_pt.hip, the
// voxel-set operators are api_voxels.hip; the ways a handle takes a new octree (adoptBuild, adoptSortedOnGrid, adoptSorted) and the one way it is edited from a
// device list (editHandle) are here.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "api_handles.h"
#include "traverse_stream.h" // (hint geometry: hintTabLevelsOf, prefixTabEntries)

static thread_local char g_err[1024] = "";
void mvrtSetError( const char* fmt, ... )
{
	va_list ap;
	va_start( ap, fmt );
	vsnprintf( g_err, sizeof( g_err ), fmt, ap );
	va_end( ap );
}
MVRT_EXPORT const char* mvrt_last_error( void ) { return g_err; }

// ---- runtime ------------------------------------------------------------------------------------------
MVRT_EXPORT int mvrt_device_count( int* count )
{
	MVRT_HIP( hipGetDeviceCount( count ) );
	return 0;
}
MVRT_EXPORT int mvrt_set_device( int device )
{
	MVRT_HIP( hipSetDevice( device ) );
	return 0;
}
MVRT_EXPORT int mvrt_device_name( char* buf, int bufLen )
{
	int dev = 0;
	MVRT_HIP( hipGetDevice( &dev ) );
	hipDeviceProp_t p;
	MVRT_HIP( hipGetDeviceProperties( &p, dev ) );
	snprintf( buf, bufLen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount );
	return 0;
}
MVRT_EXPORT int mvrt_stream_create( void** stream )
{
	hipStream_t s;
	MVRT_HIP( hipStreamCreate( &s ) );
	*stream = (void*)s;
	return 0;
}
MVRT_EXPORT int mvrt_stream_destroy( void* stream )
{
	MVRT_HIP( hipStreamDestroy( (hipStream_t)stream ) );
	return 0;
}
MVRT_EXPORT int mvrt_stream_synchronize( void* stream )
{
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	return 0;
}
MVRT_EXPORT int mvrt_device_synchronize( void )
{
	MVRT_HIP( hipDeviceSynchronize() );
	return 0;
}
MVRT_EXPORT int mvrt_malloc( void** dev, uint64_t bytes )
{
	MVRT_HIP( hipMalloc( dev, bytes ? bytes : 1 ) );
	return 0;
}
MVRT_EXPORT int mvrt_free( void* dev )
{
	if( dev ) MVRT_HIP( hipFree( dev ) );
	return 0;
}
MVRT_EXPORT int mvrt_memcpy_h2d( void* dev, const void* host, uint64_t bytes, void* stream )
{
	MVRT_HIP( hipMemcpyAsync( dev, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream ) );
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	return 0;
}
MVRT_EXPORT int mvrt_memcpy_d2d( void* dstDev, const void* srcDev, uint64_t bytes, void* stream )
{
	MVRT_HIP( hipMemcpyAsync( dstDev, srcDev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream ) );
	return 0;
}
MVRT_EXPORT int mvrt_memcpy_d2h( void* host, const void* dev, uint64_t bytes, void* stream )
{
	MVRT_HIP( hipMemcpyAsync( host, dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	return 0;
}

// failure-path tests (mvrt.h): the hook and the tallies themselves live in DevBuf::alloc / release (devbuf.h)
MVRT_EXPORT int mvrt_test_fail_allocation( int64_t nth )
{
	g_devBufFailIn = nth > 0 ? nth : 0;
	return 0;
}
MVRT_EXPORT int mvrt_test_allocation_state( uint64_t* liveBuffers, uint64_t* liveBytes, uint64_t* totalAllocs )
{
	if( liveBuffers ) *liveBuffers = g_devBufState.liveBuffers;
	if( liveBytes ) *liveBytes = g_devBufState.liveBytes;
	if( totalAllocs ) *totalAllocs = g_devBufState.totalAllocs;
	return 0;
}

// ---- IntersectorOctreeGPU (the handle itself: api_handles.h, as is why its owner is flushed or drained first) --------------------------------
static int ownerFlush( const mvrt_svo* s ) { return s && s->owner ? ptFlush( s->owner ) : 0; }
int ownerDrain( const mvrt_svo* s ) { return s && s->owner ? ptDrain( s->owner ) : 0; }

// after nodes are in place: the prefix table that shortens every nVoxelsPSum walk (voxelIndexFromPath).  7 levels = 16 MiB (measured: shade kernel 19.3 ms without, 17.2 ms with 6 levels, 16.6 ms with 7, 15.9 ms with 8 = 128 MiB, per 4 steps).
static int buildTopTable( Octree& o, hipStream_t st )
{
	const uint32_t nNodes = o.nNodes, levels = o.info.levels;
	if( !o.embedded || levels == 0 ) return 0;
	// children array (32 B per node) + behind it the prefix tables of the start below the root (traverse_stream.h): one buffer, one base register
	if( o.kids.alloc( (uint64_t)nNodes * 32 + prefixTabEntries( levels ) * 4 ) ) return 1;
	if( launchCopyKids( o.nodes.as<Node64>(), nNodes, o.kids.as<uint32_t>(), st ) ) return 1;
	if( launchBuildPrefixRefs( o.kids.as<uint32_t>(), ( nNodes - 1 ) | ( (uint32_t)o.rootMask << 24 ), hintTabLevelsOf( levels ), o.kids.as<uint32_t>() + (uint64_t)nNodes * 8, st ) )
		return 1;
	static const int envK = (int)mvrtKnob( "MVRT_TOP_LEVELS", 7 );
	uint32_t k = (uint32_t)( envK < 0 ? 0 : ( envK > 8 ? 8 : envK ) );
	if( k > levels ) k = levels;
	if( k == 0 ) return 0;
	if( o.topTable.alloc( ( 1ull << ( 3 * k ) ) * sizeof( uint2 ) ) ) return 1;
	if( launchBuildTopTable( o.nodes.as<Node64>(), nNodes - 1, k, o.topTable.as<uint2>(), st ) ) return 1;
	o.topLevels = k;
	return 0;
}

static void setBounds( mvrt_svo_info& info, const float origin[3], float dps, int gridRes )
{
	// IntersectorOctreeGPU.hpp:78-80: m_upper = origin + float3{dps,dps,dps} * (float)gridRes
	for( int k = 0; k < 3; k++ )
	{
		info.lower[k] = origin[k];
		info.upper[k] = origin[k] + dps * (float)gridRes;
	}
	info.dps = dps;
	info.gridRes = gridRes;
	info.levels = levelsOf( gridRes );
}

MVRT_EXPORT int mvrt_svo_create( mvrt_svo** out )
{
	*out = new mvrt_svo();
	return 0;
}
MVRT_EXPORT int mvrt_svo_destroy( mvrt_svo* svo )
{
	delete svo;
	return 0;
}

// The upload contract (mvrt.h): every rule on the host arrays, before any HIP call.  Rules 1 and 5 first, then rule 2 over every node in index order,
// then one walk from the root, depth by depth in discovery order, for rules 3 and 4.  The first offending node in that order is named.
MVRT_EXPORT int mvrt_svo_check_upload( const void* nodes68Host, uint32_t numberOfNodes, uint32_t numberOfVoxels, int gridRes, int embeddedMask )
{
	REQUIRE( nodes68Host && numberOfNodes > 0, "mvrt_svo_upload: empty octree" );
	REQUIRE( gridRes >= 2 && gridRes <= ( 1 << 21 ) && ( gridRes & ( gridRes - 1 ) ) == 0, "mvrt_svo_upload: rule 1: gridRes %d is not a power of two in [2, 2^21]",
			 gridRes );
	const int L = levelsOf( gridRes );
	REQUIRE( !embeddedMask || numberOfNodes < 0xFFFFFFu, "mvrt_svo_upload: rule 5: embedded masks need fewer than 0xFFFFFF nodes (IntersectorOctreeGPU.hpp:231), got %u",
			 numberOfNodes );
	const uint8_t* base = (const uint8_t*)nodes68Host;
	auto maskOf = [base]( uint32_t n ) { return (uint32_t)base[(uint64_t)n * 68]; };
	auto word = [base]( uint32_t n, uint32_t w ) // w: 1..8 children, 9..16 nVoxelsPSum
	{
		uint32_t v;
		memcpy( &v, base + (uint64_t)n * 68 + 4 * w, 4 );
		return v;
	};
	for( uint32_t n = 0; n < numberOfNodes; n++ ) // rule 2: reachable or not
	{
		const uint32_t mask = maskOf( n );
		for( uint32_t c = 0; c < 8; c++ )
		{
			const uint32_t ch = word( n, 1 + c );
			if( ch == MVRT_LEAF ) continue;
			REQUIRE( ( mask >> c ) & 1u, "mvrt_svo_upload: rule 2: node %u slot %u: child word 0x%08x where the mask bit is clear (absent children must be 0xFFFFFFFF)", n, c, ch );
			const uint32_t k = embeddedMask ? ch & 0xFFFFFFu : ch;
			REQUIRE( k < numberOfNodes, "mvrt_svo_upload: rule 2: node %u slot %u: child word 0x%08x names node %u, not below numberOfNodes %u", n, c, ch, k, numberOfNodes );
			REQUIRE( !embeddedMask || ( ch >> 24 ) == maskOf( k ),
					 "mvrt_svo_upload: rule 2: node %u slot %u: embedded mask byte 0x%02x differs from the mask 0x%02x of node %u (plain indices need embeddedMask = 0)", n, c,
					 ch >> 24, maskOf( k ), k );
		}
	}
	// rules 3 and 4: per reached node its depth << 56 | the largest nVoxelsPSum sum from the root to it (< 21 * 2^32)
	const uint64_t kSum = ( 1ull << 56 ) - 1;
	std::vector<uint64_t> seen( numberOfNodes, ~0ull );
	std::vector<uint32_t> cur( 1, numberOfNodes - 1 ), next;
	seen[numberOfNodes - 1] = 0;
	uint32_t badNode = 0, badSlot = 0;
	uint64_t badSum = 0;
	bool bad = false;
	for( uint32_t d = 0; !cur.empty(); d++ )
	{
		next.clear();
		for( const uint32_t n : cur )
		{
			const uint32_t mask = maskOf( n );
			const uint64_t s = seen[n] & kSum;
			for( uint32_t c = 0; c < 8; c++ )
			{
				if( !( ( mask >> c ) & 1u ) ) continue;
				const uint32_t ch = word( n, 1 + c );
				const uint64_t sum = s + word( n, 9 + c );
				if( ch == MVRT_LEAF )
				{
					REQUIRE( d + 1 == (uint32_t)L,
							 "mvrt_svo_upload: rule 3: node %u at depth %u holds a voxel in slot %u, %u level(s) above the last level: voxels above the last level "
							 "(coarse voxels) are not supported",
							 n, d, c, (uint32_t)L - 1 - d );
					if( sum >= numberOfVoxels && !bad )
					{
						bad = true;
						badNode = n;
						badSlot = c;
						badSum = sum;
					}
					continue;
				}
				const uint32_t k = embeddedMask ? ch & 0xFFFFFFu : ch;
				REQUIRE( d + 1 < (uint32_t)L, "mvrt_svo_upload: rule 3: node %u at depth %u has node %u in slot %u: the octree is deeper than log2(gridRes) = %d levels", n, d,
						 k, c, L );
				if( seen[k] == ~0ull )
				{
					seen[k] = ( (uint64_t)( d + 1 ) << 56 ) | sum;
					next.push_back( k );
					continue;
				}
				REQUIRE( ( seen[k] >> 56 ) == d + 1,
						 "mvrt_svo_upload: rule 3: node %u at depth %u has node %u in slot %u, which is reached at depth %u as well (a cycle or a node shared at two depths)", n, d, k,
						 c, (uint32_t)( seen[k] >> 56 ) );
				if( sum > ( seen[k] & kSum ) ) seen[k] = ( seen[k] & ~kSum ) | sum;
			}
		}
		cur.swap( next );
	}
	REQUIRE( !bad, "mvrt_svo_upload: rule 4: node %u slot %u: the nVoxelsPSum sum along a path to this voxel is %llu, not below numberOfVoxels %u", badNode, badSlot,
			 (unsigned long long)badSum, numberOfVoxels );
	return 0;
}

MVRT_EXPORT int mvrt_svo_upload( mvrt_svo* svo, const void* nodes68Host, uint32_t numberOfNodes, const void* attribs8Host, uint32_t numberOfVoxels, const float origin[3],
								 float dps, int gridRes, int hasEmission, int embeddedMask, void* stream )
{
	REQUIRE( svo && nodes68Host && numberOfNodes > 0, "mvrt_svo_upload: empty octree" );
	REQUIRE( attribs8Host || numberOfVoxels == 0, "mvrt_svo_upload: %u voxels without attributes", numberOfVoxels );
	if( mvrt_svo_check_upload( nodes68Host, numberOfNodes, numberOfVoxels, gridRes, embeddedMask ) ) return 1; // before anything is replaced
	hipStream_t st = (hipStream_t)stream;
	if( ownerDrain( svo ) ) return 1; // steps already issued keep the octree they were issued with
	svo->cleanUp();
	Octree o;
	DevBuf raw;
	if( raw.alloc( (uint64_t)numberOfNodes * 68 ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( raw.p, nodes68Host, (uint64_t)numberOfNodes * 68, hipMemcpyHostToDevice, st ) );
	if( o.nodes.alloc( (uint64_t)numberOfNodes * sizeof( Node64 ) ) || o.masks.alloc( numberOfNodes ) || o.attrs.alloc( (uint64_t)numberOfVoxels * 8 ) ) return 1;
	if( numberOfVoxels ) MVRT_HIP( hipMemcpyAsync( o.attrs.p, attribs8Host, (uint64_t)numberOfVoxels * 8, hipMemcpyHostToDevice, st ) );
	if( !embeddedMask && o.psumCold.alloc( (uint64_t)numberOfNodes * 32 ) ) return 1;
	if( launchConvertNodes( raw.as<uint8_t>(), numberOfNodes, o.nodes.as<Node64>(), o.masks.as<uint8_t>(), o.psumCold.as<uint32_t>(), embeddedMask ? 0 : 1, st ) ) return 1;
	o.nNodes = numberOfNodes;
	o.nVoxels = numberOfVoxels;
	o.hasEmission = hasEmission ? 1 : 0;
	o.embedded = embeddedMask ? 1 : 0;
	setBounds( o.info, origin, dps, gridRes );
	o.rootMask = ( (const uint8_t*)nodes68Host )[(uint64_t)( numberOfNodes - 1 ) * 68];
	if( embeddedMask ) // an uploaded octree may carry any nVoxelsPSum (mvrt.h): the popcount shortcut of the last level only for canonical ones
	{
		DevBuf bad;
		if( bad.alloc( 4 ) ) return 1;
		if( launchCheckLeafPsum( o.nodes.as<Node64>(), o.masks.as<uint8_t>(), numberOfNodes, bad.as<uint32_t>(), st ) ) return 1;
		uint32_t h = 0;
		MVRT_HIP( hipMemcpyAsync( &h, bad.p, 4, hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
		o.leafPsumIsPopcount = h ? 0u : 1u;
	}
	if( buildTopTable( o, st ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (raw is released on return)
	svo->oct = std::move( o );
	return 0;
}

// SvoDev::cellBlocks / cellEntries from the sorted voxel codes of a build (not for the tree flavour, whose traversal reports voxel indices itself)
static int buildCellIndex( Octree& o, hipStream_t st )
{
	static const int on = (int)mvrtKnob( "MVRT_CELL_INDEX", 1 );
	const uint32_t L = o.info.levels;
	if( !on || o.tree || !o.morton.p || o.nVoxels == 0 || L == 0 || L > 14u ) return 0;
	static const uint32_t blockBits = (uint32_t)mvrtKnob( "MVRT_CELL_BITS", 9 );
	const uint32_t cellBits = 3u * ( L - 1u ) < blockBits ? 3u * ( L - 1u ) : blockBits; // 8 x 8 x 8 cells per block (fewer in octrees of fewer than 4 levels)
	const uint64_t nBlockCodes = 1ull << ( 3u * ( L - 1u ) - cellBits );
	// an accelerator, not a necessity: where a table would take more than a quarter of what is free, the octree keeps the nVoxelsPSum walk
	DevBuf cnt, blocks, entries;
	size_t freeB = 0, totalB = 0;
	if( hipMemGetInfo( &freeB, &totalB ) != hipSuccess || nBlockCodes * 4 > freeB / 4 ) return 0;
	if( cnt.alloc( 4 ) || blocks.alloc( nBlockCodes * 4 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( cnt.p, 0, 4, st ) );
	MVRT_HIP( hipMemsetAsync( blocks.p, 0xFF, nBlockCodes * 4, st ) );
	if( launchNumberCellBlocks( o.morton.as<uint64_t>(), o.nVoxels, cellBits, blocks.as<uint32_t>(), cnt.as<uint32_t>(), st ) ) return 1;
	uint32_t nBlocks = 0;
	MVRT_HIP( hipMemcpyAsync( &nBlocks, cnt.p, 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	const uint64_t bytes = ( (uint64_t)nBlocks << cellBits ) * sizeof( uint2 );
	if( hipMemGetInfo( &freeB, &totalB ) != hipSuccess || bytes > freeB / 4 ) return 0;
	if( entries.alloc( bytes ) ) return 1;
	MVRT_HIP( hipMemsetAsync( entries.p, 0, bytes, st ) );
	if( launchFillCellIndex( o.morton.as<uint64_t>(), o.nVoxels, cellBits, blocks.as<uint32_t>(), entries.as<uint2>(), st ) ) return 1;
	o.cellBlocks = std::move( blocks );
	o.cellEntries = std::move( entries );
	o.cellBits = cellBits;
	return 0;
}

// The builder's arrays become the handle's octree.  What the handle still holds (build_voxels, edit_voxels: the old octree, kept while the main arrays
// were built next to it) is released before the derived tables are made; from there on a failure leaves the handle empty.
int adoptBuild( mvrt_svo* svo, SvoBuildResult& r, const float origin[3], float dps, int gridRes, int flags )
{
	Octree o( std::move( r ) );
	o.buildFlags = flags & ( MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK );
	setBounds( o.info, origin, dps, gridRes );
	svo->cleanUp();
	// default stream from here on: every builder that hands over an SvoBuildResult has ended in hipStreamSynchronize( st ) (svo_build.hip), so the arrays are complete
	MVRT_HIP( hipMemcpy( &o.rootMask, o.masks.as<uint8_t>() + ( o.nNodes - 1 ), 1, hipMemcpyDeviceToHost ) );
	if( buildTopTable( o, nullptr ) ) return 1;
	if( buildCellIndex( o, nullptr ) ) return 1;
	MVRT_HIP( hipDeviceSynchronize() ); // the derived tables stand before the call returns, whatever stream the caller traces on
	svo->oct = std::move( o );
	return 0;
}
// the same on the handle's own grid, for a build made from its own voxels (the grid is read before the old octree goes)
int adoptOnOwnGrid( mvrt_svo* svo, SvoBuildResult& r, int flags )
{
	const mvrt_svo_info info = svo->oct.info;
	return adoptBuild( svo, r, info.lower, info.dps, (int)info.gridRes, flags );
}
// The end of every in-place voxel-set call: the handle takes the sorted list an operator left (launch.h, SortedVoxels).  An unchanged list leaves the handle
// untouched; otherwise the old octree stays whole, and the handle as it was on failure, until the levels over the new list stand next to it: the owner is
// drained, the levels are built with the handle's grid and flags, totalDumped ends as an edit leaves it, and adoptBuild swaps.  The out-counts are the caller's
int adoptSorted( mvrt_svo* svo, SortedVoxels& v, hipStream_t st )
{
	if( v.unchanged( svo->oct.nVoxels ) ) return 0; // nothing changes: the handle is not touched
	if( ownerDrain( svo ) ) return 1; // steps already issued render the old scene
	const mvrt_svo_info info = svo->oct.info; // (read before the old octree goes)
	return adoptSortedOnGrid( svo, v, 0 /* as an edit leaves it */, info.lower, info.dps, (int)info.gridRes, svo->oct.buildFlags, nullptr, st );
}
// A new octree from a sorted list on a given grid (the coarsening, the resampling, adoptSorted): the levels are built next to whatever the handle holds, which may
// be the source of the list, with the list's emission flag and the caller's totalDumped, and adoptBuild swaps.  *nOut (may be null) = the voxels of the list, written
// once the levels stand.  The caller has drained the owner
int adoptSortedOnGrid( mvrt_svo* svo, SortedVoxels& v, uint64_t totalDumped, const float origin[3], float dps, int gridRes, int flags, uint64_t* nOut, hipStream_t st )
{
	SvoBuildResult r;
	if( svoBuildFromSorted( v.codes, v.attrs, v.n, gridRes, flags, st, &r ) ) return 1;
	r.hasEmission = v.hasEmission;
	r.totalDumped = totalDumped;
	if( nOut ) *nOut = v.n;
	return adoptBuild( svo, r, origin, dps, gridRes, flags );
}
// The one route of an edit from a device list of n entries (mvrt_svo_edit_voxels, the fills, the attribute transfer): the owner is drained, the edit runs on the
// handle's own list, grid and flags, and the handle ends as the edit's outcome says -- a structural edit is adopted on the handle's grid, an attribute-only one has
// written in place.  accepts: the outcomes the caller's list can have (EDIT_STRUCTURAL | EDIT_ATTRIBUTES); the other one is an internal error, worded for the one
// caller that can meet it.  ownXyz / ownAttribs (may be null): the caller's scratch behind xyz / attribs, released before the levels are adopted
int editHandle( mvrt_svo* svo, const char* who, int accepts, const uint32_t* xyz, const uint32_t* attribs, const uint8_t* ops, uint64_t n, DevBuf* ownXyz, DevBuf* ownAttribs,
				hipStream_t st )
{
	if( ownerDrain( svo ) ) return 1; // steps already issued render the old scene; an attribute-only edit writes in place
	Octree& o = svo->oct;
	o.lod = LodPyramid(); // the edit may write attributes in place: the pyramid does not outlive the voxels it describes
	SvoBuildResult r;
	int structural = 0;
	uint32_t he = 0;
	if( svoEditVoxels( o.morton.as<uint64_t>(), o.attrs.as<uint2>(), o.nVoxels, xyz, attribs, ops, n, (int)o.info.gridRes, o.buildFlags, st, &r, &structural, &he ) ) return 1;
	REQUIRE( structural || ( accepts & EDIT_ATTRIBUTES ), "%s: internal error: the enclosed cells hold voxels", who ); // (a fill: every cell is an insert)
	REQUIRE( !structural || ( accepts & EDIT_STRUCTURAL ), "%s: internal error: the voxels of the handle are not its voxels", who ); // (a transfer: every entry is a voxel)
	if( !structural )
	{
		o.totalDumped = 0;
		o.hasEmission = he;
		return 0;
	}
	if( ownXyz ) ownXyz->release();
	if( ownAttribs ) ownAttribs->release();
	return adoptOnOwnGrid( svo, r, o.buildFlags );
}
MVRT_EXPORT int mvrt_svo_build_ex( mvrt_svo* svo, const float* verticesHost, const float* vcolorsHost, const float* vemissionsHost, uint64_t nVertices, void* stream,
								   const float origin[3], float dps, int gridRes, int flags )
{
	REQUIRE( svo && verticesHost && nVertices >= 3 && nVertices % 3 == 0, "mvrt_svo_build: need 3*k vertices" );
	REQUIRE( levelsOf( gridRes ) > 0, "gridRes %d is not a power of two >= 2 (IntersectorOctreeGPU.hpp:48-51)", gridRes );
	hipStream_t st = (hipStream_t)stream;
	if( ownerDrain( svo ) ) return 1; // steps already issued keep the octree they were issued with
	svo->cleanUp(); // :53
	SvoBuildResult r;
	if( svoBuildFromTriangles( verticesHost, vcolorsHost, vemissionsHost, nVertices, mk3( origin[0], origin[1], origin[2] ), dps, gridRes, flags, st, &r ) ) return 1;
	return adoptBuild( svo, r, origin, dps, gridRes, flags );
}
MVRT_EXPORT int mvrt_svo_build( mvrt_svo* svo, const float* verticesHost, const float* vcolorsHost, const float* vemissionsHost, uint64_t nVertices, void* stream,
								const float origin[3], float dps, int gridRes )
{
	return mvrt_svo_build_ex( svo, verticesHost, vcolorsHost, vemissionsHost, nVertices, stream, origin, dps, gridRes, 0 );
}
MVRT_EXPORT int mvrt_svo_build_synthetic( mvrt_svo* svo, int gridRes, uint64_t nRandomVoxels, uint64_t seed, const float origin[3], float dps, int flags, void* stream )
{
	REQUIRE( svo, "null argument" );
	REQUIRE( levelsOf( gridRes ) > 0 && gridRes <= ( 1 << 21 ), "gridRes %d is not a power of two in [2, 2^21]", gridRes );
	if( ownerDrain( svo ) ) return 1;
	svo->cleanUp();
	SvoBuildResult r;
	if( svoBuildSynthetic( nRandomVoxels, seed, gridRes, flags, (hipStream_t)stream, &r ) ) return 1;
	return adoptBuild( svo, r, origin, dps, gridRes, flags );
}

// Voxel lists.  Arguments are checked on the host first, the device checks (coordinates, ops) come before anything is replaced, and the new list and levels are
// built next to the old octree: every failure up to there leaves the handle as it was.  adoptBuild then releases the old octree; a failure after that leaves it empty.
MVRT_EXPORT int mvrt_svo_build_voxels( mvrt_svo* svo, const uint32_t* xyzDev, const uint32_t* attribsDev, uint64_t n, const float origin[3], float dps, int gridRes, int flags,
									   void* stream )
{
	REQUIRE( svo, "mvrt_svo_build_voxels: null handle" );
	REQUIRE( xyzDev && origin, "mvrt_svo_build_voxels: null coordinates or origin" );
	REQUIRE( n >= 1 && n < 0xFFFFFFFFull, "mvrt_svo_build_voxels: voxel count %llu is not in [1, 2^32-2]", (unsigned long long)n );
	REQUIRE( levelsOf( gridRes ) > 0 && gridRes <= ( 1 << 21 ), "mvrt_svo_build_voxels: gridRes %d is not a power of two in [2, 2^21]", gridRes );
	REQUIRE_BUILD_FLAGS( "mvrt_svo_build_voxels", flags );
	hipStream_t st = (hipStream_t)stream;
	if( ownerDrain( svo ) ) return 1; // steps already issued keep the octree they were issued with
	SvoBuildResult r;
	if( svoBuildFromVoxels( xyzDev, attribsDev, n, gridRes, flags, st, &r ) ) return 1;
	return adoptBuild( svo, r, origin, dps, gridRes, flags );
}
MVRT_EXPORT int mvrt_svo_edit_voxels( mvrt_svo* svo, const uint32_t* xyzDev, const uint32_t* attribsDev, const uint8_t* opsDev, uint64_t n, void* stream )
{
	REQUIRE( svo, "mvrt_svo_edit_voxels: null handle" );
	REQUIRE( !svo->empty(), "mvrt_svo_edit_voxels: no octree (build first)" );
	REQUIRE( svo->oct.morton.p, "mvrt_svo_edit_voxels: an uploaded octree keeps no Morton codes; only octrees built by this library can be edited" );
	REQUIRE( xyzDev, "mvrt_svo_edit_voxels: null coordinates" );
	REQUIRE( n >= 1 && n < 0xFFFFFFFFull, "mvrt_svo_edit_voxels: entry count %llu is not in [1, 2^32-2]", (unsigned long long)n );
	return editHandle( svo, "mvrt_svo_edit_voxels", EDIT_STRUCTURAL | EDIT_ATTRIBUTES, xyzDev, attribsDev, opsDev, n, nullptr, nullptr, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_svo_read_voxels( const mvrt_svo* svo, uint32_t* xyzDev, uint32_t* attribsDev, void* stream )
{
	REQUIRE( svo, "mvrt_svo_read_voxels: null handle" );
	REQUIRE( !svo->empty(), "mvrt_svo_read_voxels: no octree (build first)" );
	REQUIRE( svo->oct.morton.p, "mvrt_svo_read_voxels: an uploaded octree keeps no Morton codes" );
	return svoReadVoxels( svo->oct.morton.as<uint64_t>(), svo->oct.attrs.as<uint2>(), svo->oct.nVoxels, xyzDev, attribsDev, (hipStream_t)stream );
}

// The voxels of whatever the handle holds (kernels_walk.hip).  A handle that keeps Morton codes is answered from them (entry i is voxel i: the tree flavour
// has nothing else to walk); every other octree is walked from the root.  Both give the same bytes.  The caller's arrays are written by the last launch alone,
// behind every allocation and check.
static WalkSource walkSource( const Octree& o )
{
	WalkSource s;
	s.nodes = o.nodes.as<Node64>();
	s.masks = o.masks.as<uint8_t>();
	s.psumCold = o.psumCold.as<uint32_t>();
	s.nNodes = o.nNodes;
	s.levels = o.info.levels;
	s.embedded = o.embedded;
	s.rootMask = o.rootMask;
	return s;
}
MVRT_EXPORT int mvrt_svo_walk_voxels( const mvrt_svo* svo, uint64_t capacity, uint32_t* xyzDev, uint32_t* vIndexDev, uint32_t* attribsDev, uint64_t* nOut, void* stream )
{
	REQUIRE( svo, "mvrt_svo_walk_voxels: null handle" );
	REQUIRE( !svo->empty(), "mvrt_svo_walk_voxels: no octree (build or upload first)" );
	const Octree& o = svo->oct;
	hipStream_t st = (hipStream_t)stream;
	const bool fill = xyzDev || vIndexDev || attribsDev;
	WalkResult w;
	if( o.morton.p ) w.n = o.nVoxels;
	else if( walkPaths( walkSource( o ), fill, capacity, &w, st ) ) return 1;
	if( nOut ) *nOut = w.n;
	const int tail = listingTail( "mvrt_svo_walk_voxels", "capacity", "voxels of the octree", !fill, capacity, w.n );
	if( tail != LISTING_WRITE ) return tail;
	if( launchWalkGather( o.morton.p ? o.morton.as<uint64_t>() : w.codes.as<uint64_t>(), o.morton.p ? nullptr : w.vIndex.as<uint32_t>(), o.attrs.as<uint2>(), o.nVoxels,
						  w.n, xyzDev, vIndexDev, attribsDev, st ) )
		return 1;
	MVRT_HIP( hipStreamSynchronize( st ) ); // (the scratch is released on return)
	return 0;
}
// The handle's octree becomes the one mvrt_svo_build_voxels would build from its walked voxels.  Refusals come first, the new arrays are built next to the old
// octree: every failure up to adoptBuild leaves the handle as it was (adoptBuild itself: see there).
MVRT_EXPORT int mvrt_svo_rebuild( mvrt_svo* svo, int flags, void* stream )
{
	REQUIRE( svo, "mvrt_svo_rebuild: null handle" );
	REQUIRE( !svo->empty(), "mvrt_svo_rebuild: no octree (build or upload first)" );
	REQUIRE_BUILD_FLAGS( "mvrt_svo_rebuild", flags );
	hipStream_t st = (hipStream_t)stream;
	if( ownerDrain( svo ) ) return 1; // steps already issued keep the octree they were issued with
	const Octree& o = svo->oct;
	const mvrt_svo_info info = o.info;
	DevBuf morton, attrs;
	uint64_t n = 0;
	if( o.morton.p ) // a flavour change of a built octree: its list as it is
	{
		n = o.nVoxels;
		if( morton.alloc( n * 8 ) || attrs.alloc( n * 8 ) ) return 1;
		MVRT_HIP( hipMemcpyAsync( morton.p, o.morton.p, n * 8, hipMemcpyDeviceToDevice, st ) );
		MVRT_HIP( hipMemcpyAsync( attrs.p, o.attrs.p, n * 8, hipMemcpyDeviceToDevice, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
	}
	else
	{
		WalkResult w;
		if( walkPaths( walkSource( o ), true, 0xFFFFFFFEull, &w, st ) ) return 1;
		n = w.n;
		REQUIRE( n >= 1, "mvrt_svo_rebuild: the octree holds no voxel" );
		REQUIRE( n < 0xFFFFFFFFull, "mvrt_svo_rebuild: %llu voxels exceed the 32-bit index range of the builder", (unsigned long long)n );
		if( attrs.alloc( n * 8 ) ) return 1;
		if( launchWalkGather( w.codes.as<uint64_t>(), w.vIndex.as<uint32_t>(), o.attrs.as<uint2>(), o.nVoxels, n, nullptr, nullptr, attrs.as<uint32_t>(), st ) ) return 1;
		MVRT_HIP( hipStreamSynchronize( st ) ); // (the vIndex array is released at scope end)
		morton = std::move( w.codes );
	}
	SvoBuildResult r;
	if( svoBuildFromSorted( morton, attrs, (uint32_t)n, (int)info.gridRes, flags, st, &r ) ) return 1;
	r.hasEmission = o.hasEmission; // the handle's flag, not recomputed: the scene renders as before
	return adoptOnOwnGrid( svo, r, flags );
}

MVRT_EXPORT int mvrt_svo_get_info( const mvrt_svo* svo, mvrt_svo_info* info )
{
	REQUIRE( svo && info, "null argument" );
	const Octree& o = svo->oct;
	*info = o.info;
	info->numberOfNodes = o.nNodes;
	info->numberOfVoxels = o.nVoxels;
	info->hasEmission = o.hasEmission;
	info->embeddedMask = o.embedded;
	info->totalDumpedVoxels = o.totalDumped;
	info->emissionScale = svo->emissionScale;
	info->flavour = o.tree ? MVRT_FLAVOUR_TREE : ( info->embeddedMask ? MVRT_FLAVOUR_EMBEDDED : MVRT_FLAVOUR_PLAIN );
	info->reserved = 0;
	return 0;
}
MVRT_EXPORT uint64_t mvrt_svo_traversal_bytes( const mvrt_svo* svo )
{
	if( !svo || svo->empty() ) return 0;
	const Octree& o = svo->oct;
	const uint64_t n = o.nNodes;
	if( o.tree ) return (uint64_t)o.nBricks * sizeof( uint4 ) + n * 5;
	return n * sizeof( Node64 ) + n + ( o.psumCold.p ? n * 32 : 0 ) + o.topTable.bytes + o.kids.bytes + o.cellBlocks.bytes + o.cellEntries.bytes;
}
MVRT_EXPORT const void* mvrt_svo_node_buffer_dev( const mvrt_svo* svo ) { return svo ? svo->oct.nodes.p : nullptr; }
MVRT_EXPORT const void* mvrt_svo_attribute_buffer_dev( const mvrt_svo* svo ) { return svo ? svo->oct.attrs.p : nullptr; }
MVRT_EXPORT int mvrt_svo_device_view( const mvrt_svo* svo, mvrt_device_octree* out )
{
	REQUIRE( svo && out, "mvrt_svo_device_view: null argument" );
	REQUIRE( !svo->empty(), "mvrt_svo_device_view: no octree (build or upload first)" );
	REQUIRE( !svo->oct.tree, "mvrt_svo_device_view: tree-flavour octrees (MVRT_FLAVOUR_TREE) are not supported by the device API" );
	REQUIRE( svo->oct.info.levels <= MVRT_DEVICE_MAX_LEVELS, "mvrt_svo_device_view: %u levels, the device API supports at most %d", svo->oct.info.levels,
			 MVRT_DEVICE_MAX_LEVELS );
	const SvoDev d = svo->dev();
	mvrt_device_octree v;
	memset( &v, 0, sizeof( v ) );
	v.structBytes = sizeof( mvrt_device_octree );
	v.flavour = d.embedded ? MVRT_FLAVOUR_EMBEDDED : MVRT_FLAVOUR_PLAIN;
	v.nodes = (uint64_t)(uintptr_t)d.nodes;
	v.kids = (uint64_t)(uintptr_t)d.kids;
	v.masks = (uint64_t)(uintptr_t)d.masks;
	v.psumCold = (uint64_t)(uintptr_t)d.psumCold;
	v.attrs = (uint64_t)(uintptr_t)d.attrs;
	v.cellBlocks = (uint64_t)(uintptr_t)d.cellBlocks;
	v.cellEntries = d.cellBlocks ? (uint64_t)(uintptr_t)d.cellEntries : 0;
	v.lower[0] = d.lower.x; v.lower[1] = d.lower.y; v.lower[2] = d.lower.z;
	v.upper[0] = d.upper.x; v.upper[1] = d.upper.y; v.upper[2] = d.upper.z;
	v.dps = d.dps;
	v.emissionScale = d.emissionScale;
	v.hasEmission = d.hasEmission;
	v.levels = d.levels;
	v.numberOfNodes = d.nNodes;
	v.numberOfVoxels = d.nVoxels;
	v.rootIndex = d.rootIndex;
	v.rootMask = d.rootMask;
	v.treeRoot = 0;
	v.cellBits = d.cellBlocks ? d.cellBits : 0;
	*out = v;
	return 0;
}
MVRT_EXPORT int mvrt_svo_set_emission_scale( mvrt_svo* svo, float scale )
{
	REQUIRE( svo, "null argument" );
	if( ownerFlush( svo ) ) return 1; // pending steps are launched with the scale they were issued under
	svo->emissionScale = scale;
	return 0;
}
MVRT_EXPORT int mvrt_svo_download( const mvrt_svo* svo, void* nodes68Host, void* attribs8Host, uint64_t* mortonHost, void* stream )
{
	REQUIRE( svo && !svo->empty(), "no octree" );
	const Octree& o = svo->oct;
	const uint32_t nNodes = o.nNodes, nVoxels = o.nVoxels;
	hipStream_t st = (hipStream_t)stream;
	if( nodes68Host )
	{
		DevBuf raw;
		if( raw.alloc( (uint64_t)nNodes * 68 ) ) return 1;
		if( o.tree )
		{
			if( launchTreeTo68( o.masks.as<uint8_t>(), o.treeFirst.as<uint32_t>(), o.treeLevelBase, o.treeLevelCount, (int)o.info.levels, nNodes, nVoxels, raw.as<uint8_t>(), st ) ) return 1;
		}
		else if( launchNodesTo68( o.nodes.as<Node64>(), o.masks.as<uint8_t>(), o.psumCold.as<uint32_t>(), nNodes, raw.as<uint8_t>(), o.embedded ? 0 : 1, st ) ) return 1;
		MVRT_HIP( hipMemcpyAsync( nodes68Host, raw.p, raw.bytes, hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
	}
	if( attribs8Host ) MVRT_HIP( hipMemcpyAsync( attribs8Host, o.attrs.p, (uint64_t)nVoxels * 8, hipMemcpyDeviceToHost, st ) );
	if( mortonHost )
	{
		REQUIRE( o.morton.p, "morton codes are only kept by mvrt_svo_build" );
		MVRT_HIP( hipMemcpyAsync( mortonHost, o.morton.p, (uint64_t)nVoxels * 8, hipMemcpyDeviceToHost, st ) );
	}
	MVRT_HIP( hipStreamSynchronize( st ) );
	return 0;
}

static int traceBatch( const char* who, const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
					   const float* rdzDev, const uint8_t* isShadowDev, const uint64_t* originVoxelMortonDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev, uint32_t* descentsDev,
					   void* stream )
{
	REQUIRE( svo && !svo->empty(), "%s: no octree (build or upload first)", who );
	REQUIRE( tDev, "%s: t output is required", who );
	if( svo->ensureWorkspace( vIndexDev ? n : 0 ) ) return 1;
	return launchTraceBatch( svo->dev(), svo->work.ws, n, roxDev, royDev, rozDev, rdxDev, rdyDev, rdzDev, isShadowDev, tDev, nMajorDev, vIndexDev, descentsDev, (hipStream_t)stream,
							 originVoxelMortonDev );
}
MVRT_EXPORT int mvrt_trace_batch( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
								  const float* rdzDev, const uint8_t* isShadowDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev, uint32_t* descentsDev, void* stream )
{
	return traceBatch( "mvrt_trace_batch", svo, n, roxDev, royDev, rozDev, rdxDev, rdyDev, rdzDev, isShadowDev, nullptr, tDev, nMajorDev, vIndexDev, descentsDev, stream );
}
MVRT_EXPORT int mvrt_trace_batch_hinted( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
										 const float* rdzDev, const uint8_t* isShadowDev, const uint64_t* originVoxelMortonDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev,
										 uint32_t* descentsDev, void* stream )
{
	return traceBatch( "mvrt_trace_batch_hinted", svo, n, roxDev, royDev, rozDev, rdxDev, rdyDev, rdzDev, isShadowDev, originVoxelMortonDev, tDev, nMajorDev, vIndexDev, descentsDev,
					   stream );
}

// Distance-limited rays and the occlusion bake (kernels_range.hip): the per-lane walk of include/mvrt/device.hpp, so the flavours of mvrt_svo_device_view.
// Arguments are checked first, on the host, then the handle.
static int rangeView( const mvrt_svo* svo, const char* who, mvrt_device_octree* view )
{
	REQUIRE( !svo->oct.tree, "%s: tree-flavour octrees (MVRT_FLAVOUR_TREE) are not supported", who );
	return mvrt_svo_device_view( svo, view );
}
MVRT_EXPORT int mvrt_trace_batch_range( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
										const float* rdzDev, const uint8_t* isShadowDev, const float* tMaxDev, float* tDev, int32_t* nMajorDev, uint32_t* vIndexDev,
										uint32_t* descentsDev, void* stream )
{
	REQUIRE( tMaxDev, "mvrt_trace_batch_range: tMaxDev is required (one limit per ray)" );
	REQUIRE( tDev, "mvrt_trace_batch_range: t output is required" );
	REQUIRE( n == 0 || ( roxDev && royDev && rozDev && rdxDev && rdyDev && rdzDev ), "mvrt_trace_batch_range: null ray array" );
	REQUIRE( svo && !svo->empty(), "mvrt_trace_batch_range: no octree (build or upload first)" );
	mvrt_device_octree view;
	if( rangeView( svo, "mvrt_trace_batch_range", &view ) ) return 1;
	return launchTraceRange( view, n, roxDev, royDev, rozDev, rdxDev, rdyDev, rdzDev, isShadowDev, tMaxDev, tDev, nMajorDev, vIndexDev, descentsDev, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_ao_directions( int samples, float* dirsHost )
{
	REQUIRE( aoSamplesOk( samples ), "mvrt_ao_directions: samples = %d is not a power of two in [1, 256]", samples );
	REQUIRE( dirsHost, "mvrt_ao_directions: null output" );
	aoDirections( samples, dirsHost );
	return 0;
}
MVRT_EXPORT int mvrt_svo_surface_ao( const mvrt_svo* svo, uint64_t nFaces, const uint32_t* faceVoxelDev, const uint8_t* faceDirDev, int samples, float radius,
									 uint16_t* openDev, void* stream )
{
	REQUIRE( aoSamplesOk( samples ), "mvrt_svo_surface_ao: samples = %d is not a power of two in [1, 256]", samples );
	REQUIRE( radius > 0.0f, "mvrt_svo_surface_ao: radius %g is not greater than 0 (MVRT_MAX_FLOAT or +inf = unlimited)", (double)radius );
	REQUIRE( nFaces == 0 || ( faceVoxelDev && faceDirDev && openDev ), "mvrt_svo_surface_ao: null faceVoxelDev, faceDirDev or openDev" );
	SurfaceSource s;
	if( surfaceSource( svo, "mvrt_svo_surface_ao", &s ) ) return 1;
	mvrt_device_octree view;
	if( rangeView( svo, "mvrt_svo_surface_ao", &view ) ) return 1;
	return surfaceAo( view, s.morton, nFaces, faceVoxelDev, faceDirDev, samples, radius, openDev, (hipStream_t)stream );
}

// Cone-limited rays (kernels_lod.hip): the same per-lane walk, so the octrees of rangeView; the pyramid is asked for only where an output needs it
MVRT_EXPORT int mvrt_trace_batch_cone( const mvrt_svo* svo, uint64_t n, const float* roxDev, const float* royDev, const float* rozDev, const float* rdxDev, const float* rdyDev,
									   const float* rdzDev, const float* coneADev, const float* coneBDev, float* tDev, int32_t* nMajorDev, uint32_t* levelDev, uint64_t* cellCodeDev,
									   uint32_t* indexDev, uint32_t* attribDev, uint32_t* descentsDev, void* stream )
{
	REQUIRE( coneADev && coneBDev, "mvrt_trace_batch_cone: coneADev and coneBDev are required (one cone per ray)" );
	REQUIRE( tDev, "mvrt_trace_batch_cone: t output is required" );
	REQUIRE( n == 0 || ( roxDev && royDev && rozDev && rdxDev && rdyDev && rdzDev ), "mvrt_trace_batch_cone: null ray array" );
	REQUIRE( svo && !svo->empty(), "mvrt_trace_batch_cone: no octree (build or upload first)" );
	mvrt_device_octree view;
	if( rangeView( svo, "mvrt_trace_batch_cone", &view ) ) return 1;
	mvrt_device_lod lod;
	const bool needLod = indexDev || attribDev;
	REQUIRE( !needLod || svo->oct.lod.ready, "mvrt_trace_batch_cone: %s needs the attribute pyramid (mvrt_svo_lod_prepare first)", indexDev ? "indexDev" : "attribDev" );
	if( needLod && mvrt_svo_lod_view( svo, &lod ) ) return 1;
	return launchTraceCone( view, needLod ? &lod : nullptr, n, roxDev, royDev, rozDev, rdxDev, rdyDev, rdzDev, coneADev, coneBDev, tDev, nMajorDev, levelDev, cellCodeDev, indexDev,
							attribDev, descentsDev, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_render_primary_lod( const mvrt_svo* svo, const float camera[15], int width, int height, float lodScale, int showVertexColor, uint8_t* rgbaDev, float* tDev,
										 int32_t* nMajorDev, uint32_t* levelDev, uint32_t* descentsDev, void* stream )
{
	REQUIRE( camera, "mvrt_render_primary_lod: null camera" );
	REQUIRE( width > 0 && height > 0, "mvrt_render_primary_lod: bad resolution %dx%d", width, height );
	REQUIRE( svo && !svo->empty(), "mvrt_render_primary_lod: no octree (build or upload first)" );
	mvrt_device_octree view;
	if( rangeView( svo, "mvrt_render_primary_lod", &view ) ) return 1;
	mvrt_device_lod lod;
	const bool needLod = showVertexColor && rgbaDev;
	REQUIRE( !needLod || svo->oct.lod.ready, "mvrt_render_primary_lod: showVertexColor needs the attribute pyramid (mvrt_svo_lod_prepare first)" );
	if( needLod && mvrt_svo_lod_view( svo, &lod ) ) return 1;
	const float coneB = lodScale * ( ( 2.0f * camera[12] ) / (float)height ); // lodScale pixels' width at rd . front = 1
	return launchRenderLod( view, needLod ? &lod : nullptr, camera, width, height, coneB, (uchar4*)rgbaDev, tDev, nMajorDev, levelDev, descentsDev, (hipStream_t)stream );
}

MVRT_EXPORT int mvrt_trace_batch_host( const mvrt_svo* svo, uint64_t n, const float* roHost, const float* rdHost, const uint8_t* isShadowHost, float* tHost,
									   int32_t* nMajorHost, uint32_t* vIndexHost, uint32_t* descentsHost )
{
	REQUIRE( svo && !svo->empty(), "mvrt_trace_batch_host: no octree" );
	if( n == 0 ) return 0;
	std::vector<float> soa( n * 6 );
	for( uint64_t i = 0; i < n; i++ )
		for( int k = 0; k < 3; k++ )
		{
			soa[k * n + i] = roHost[i * 3 + k];
			soa[( 3 + k ) * n + i] = rdHost[i * 3 + k];
		}
	DevBuf in, sh, t, nm, vi, de;
	if( in.alloc( n * 24 ) || t.alloc( n * 4 ) || nm.alloc( n * 4 ) || vi.alloc( n * 4 ) || de.alloc( n * 4 ) ) return 1;
	MVRT_HIP( hipMemcpy( in.p, soa.data(), n * 24, hipMemcpyHostToDevice ) ); // (no stream argument: default stream throughout, ended by the hipDeviceSynchronize below)
	if( isShadowHost )
	{
		if( sh.alloc( n ) ) return 1;
		MVRT_HIP( hipMemcpy( sh.p, isShadowHost, n, hipMemcpyHostToDevice ) ); // (default stream, as above)
	}
	const float* b = in.as<float>();
	if( svo->ensureWorkspace( n ) ) return 1;
	if( launchTraceBatch( svo->dev(), svo->work.ws, n, b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n, isShadowHost ? sh.as<uint8_t>() : nullptr, t.as<float>(), nm.as<int32_t>(),
						  vi.as<uint32_t>(), de.as<uint32_t>(), 0 ) )
		return 1;
	MVRT_HIP( hipDeviceSynchronize() );
	// default stream, the four downloads: behind the hipDeviceSynchronize above
	MVRT_HIP( hipMemcpy( tHost, t.p, n * 4, hipMemcpyDeviceToHost ) );
	if( nMajorHost ) MVRT_HIP( hipMemcpy( nMajorHost, nm.p, n * 4, hipMemcpyDeviceToHost ) );
	if( vIndexHost ) MVRT_HIP( hipMemcpy( vIndexHost, vi.p, n * 4, hipMemcpyDeviceToHost ) );
	if( descentsHost ) MVRT_HIP( hipMemcpy( descentsHost, de.p, n * 4, hipMemcpyDeviceToHost ) );
	return 0;
}

MVRT_EXPORT int mvrt_render_primary( const mvrt_svo* svo, const float camera[15], int width, int height, int showVertexColor, uint8_t* rgbaDev, float* tDev,
									 int32_t* nMajorDev, uint32_t* vIndexDev, uint32_t* descentsDev, void* stream )
{
	REQUIRE( svo && !svo->empty(), "mvrt_render_primary: no octree" );
	REQUIRE( width > 0 && height > 0, "bad resolution %dx%d", width, height );
	if( svo->ensureWorkspace( ( vIndexDev || showVertexColor ) ? (uint64_t)width * height : 0 ) ) return 1;
	if( !tDev && ( vIndexDev || showVertexColor ) ) tDev = (float*)( svo->work.ws.paths + svo->work.ws.pathCap ); // the resolve pass needs t
	return launchRenderPrimary( svo->dev(), svo->work.ws, cameraFrom15( camera ), width, height, showVertexColor, (uchar4*)rgbaDev, tDev, nMajorDev, vIndexDev, descentsDev,
								(hipStream_t)stream );
}

// CameraPinhole::initFromPerspective, renderCommon.hpp:21-35 (glm column-major matrices)
MVRT_EXPORT int mvrt_camera_from_matrices( const float view[16], const float proj[16], float focus, float lensR, float cameraOut[15] )
{
	f3 r0 = mk3( view[0], view[4], view[8] ); // rows of mat3(view) = columns of its transpose
	f3 r1 = mk3( view[1], view[5], view[9] );
	f3 r2 = mk3( view[2], view[6], view[10] );
	f3 v = mk3( view[12], view[13], view[14] );
	f3 m = mk3( r0.x * v.x + r1.x * v.y + r2.x * v.z, r0.y * v.x + r1.y * v.y + r2.y * v.z, r0.z * v.x + r1.z * v.y + r2.z * v.z );
	CameraPinhole c;
	c.front = mk3( -r2.x, -r2.y, -r2.z );
	c.up = r1;
	c.right = r0;
	c.o = mk3( -m.x, -m.y, -m.z );
	c.tanHthetaY = 1.0f / proj[5];
	c.lensR = lensR;
	c.focus = focus;
	memcpy( cameraOut, &c, sizeof( c ) );
	return 0;
}

MVRT_EXPORT int mvrt_compact_indices( const uint8_t* keepDev, uint64_t n, uint32_t* dstIndexDev, uint32_t* keptDev, void* stream )
{
	if( n == 0 )
	{
		if( keptDev ) MVRT_HIP( hipMemsetAsync( keptDev, 0, 4, (hipStream_t)stream ) );
		return 0;
	}
	DevBuf scratch;
	if( scratch.alloc( ( scanCountEntries( n ) + scanTileEntries( n ) ) * 4 ) ) return 1; // block counts, then the tile sums of the scan (launch.h)
	if( launchCompactIndices( keepDev, n, dstIndexDev, keptDev, scratch.as<uint32_t>(), (hipStream_t)stream ) ) return 1;
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) ); // scratch is freed on return
	return 0;
}
