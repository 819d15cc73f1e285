// IntersectorOctreeGPU.hpp -- header-only C++ mirror of the reference's host struct
// (reference IntersectorOctreeGPU.hpp:21-275) over the C-ABI in include/mvrt.h.
//
// Same member names, same call order, same void signatures.  What a reference call site has to change:
//   * glm::vec3 vectors arrive as `const std::vector<mvrt::vec3>&` (any 3-float POD of the same layout,
//     glm::vec3 included -- reinterpret_cast is enough: the reference itself static_asserts
//     sizeof(glm::vec3) == sizeof(float3), IntersectorOctreeGPU.hpp:61);
//   * the `Shader* voxKernel` argument is accepted and ignored (kernels are precompiled into libmvrt_hip.so);
//   * `oroStream` becomes `void*` (a hipStream_t).
// Failures abort(), like the reference (hipUtil.hpp:18-22, IntersectorOctreeGPU.hpp:48-51).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mvrt.h"

namespace mvrt
{
struct vec3
{
	float x, y, z;
};
inline void check( int rc, const char* what )
{
	if( rc != 0 )
	{
		std::fprintf( stderr, "%s failed: %s\n", what, mvrt_last_error() );
		std::abort();
	}
}

struct IntersectorOctreeGPU
{
	IntersectorOctreeGPU() { check( mvrt_svo_create( &m_handle ), "mvrt_svo_create" ); }
	explicit IntersectorOctreeGPU( mvrt_svo* borrowed ) : m_handle( borrowed ), m_owned( false ) {}
	~IntersectorOctreeGPU()
	{
		if( m_owned && m_handle ) mvrt_svo_destroy( m_handle );
	}
	IntersectorOctreeGPU( const IntersectorOctreeGPU& ) = delete;
	void operator=( const IntersectorOctreeGPU& ) = delete;

	// reference :26-38
	void cleanUp()
	{
		if( m_owned )
		{
			mvrt_svo_destroy( m_handle );
			check( mvrt_svo_create( &m_handle ), "mvrt_svo_create" );
		}
		refresh();
	}

	// reference :40-47 -- build(vertices, vcolors, vemissions, Shader*, stream, origin, dps, gridRes)
	// (buildFlags: MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK | MVRT_BUILD_CONSERVATIVE -- the reference's compile-time switches
	// ENABLE_GPU_DAG / ENABLE_EMBEDED_MASK, voxCommon.hpp:5-9, and VTContext's sixSeparating flag, as run-time options; 0 = the reference's defaults)
	template <class V3>
	void build( const std::vector<V3>& vertices, const std::vector<V3>& vcolors, const std::vector<V3>& vemissions, void* /*voxKernel*/, void* stream, V3 origin, float dps,
				int gridRes, int buildFlags = 0 )
	{
		static_assert( sizeof( V3 ) == 3 * sizeof( float ), "vertex type must be 3 packed floats" );
		const float o[3] = { origin.x, origin.y, origin.z };
		check( mvrt_svo_build_ex( m_handle, reinterpret_cast<const float*>( vertices.data() ), vcolors.empty() ? nullptr : reinterpret_cast<const float*>( vcolors.data() ),
								  vemissions.empty() ? nullptr : reinterpret_cast<const float*>( vemissions.data() ), vertices.size(), stream, o, dps, gridRes, buildFlags ),
			   "IntersectorOctreeGPU::build" );
		refresh();
	}

	// adopt an octree built on the CPU (IntersectorOctree::buildDAGReference), reference 68-byte nodes
	void upload( const void* nodes68, uint32_t numberOfNodes, const void* attribs8, uint32_t numberOfVoxels, vec3 origin, float dps, int gridRes, bool hasEmission,
				 bool embeddedMask, void* stream )
	{
		const float o[3] = { origin.x, origin.y, origin.z };
		check( mvrt_svo_upload( m_handle, nodes68, numberOfNodes, attribs8, numberOfVoxels, o, dps, gridRes, hasEmission, embeddedMask, stream ), "mvrt_svo_upload" );
		refresh();
	}
	// the upload contract (mvrt.h) on host arrays alone, no GPU call: true when upload() would accept them; else false and mvrt_last_error() says why
	static bool checkUpload( const void* nodes68, uint32_t numberOfNodes, uint32_t numberOfVoxels, int gridRes, bool embeddedMask )
	{
		return mvrt_svo_check_upload( nodes68, numberOfNodes, numberOfVoxels, gridRes, embeddedMask ) == 0;
	}

	// voxel lists (mvrt_svo_build_voxels / mvrt_svo_edit_voxels / mvrt_svo_read_voxels): device arrays of xyz (3 x u32 per voxel) and VoxelAttirb (2 x u32 per voxel,
	// nullptr = white, no emission); ops: MVRT_VOXEL_SET / MVRT_VOXEL_REMOVE per entry (nullptr = all SET), the last entry per voxel wins
	void buildFromVoxels( const uint32_t* xyzDev, const uint32_t* attribsDev, uint64_t n, vec3 origin, float dps, int gridRes, int buildFlags, void* stream )
	{
		const float o[3] = { origin.x, origin.y, origin.z };
		check( mvrt_svo_build_voxels( m_handle, xyzDev, attribsDev, n, o, dps, gridRes, buildFlags, stream ), "IntersectorOctreeGPU::buildFromVoxels" );
		refresh();
	}
	void editVoxels( const uint32_t* xyzDev, const uint32_t* attribsDev, const uint8_t* opsDev, uint64_t n, void* stream )
	{
		check( mvrt_svo_edit_voxels( m_handle, xyzDev, attribsDev, opsDev, n, stream ), "IntersectorOctreeGPU::editVoxels" );
		refresh();
	}
	void readVoxels( uint32_t* xyzDev, uint32_t* attribsDev, void* stream ) const
	{
		check( mvrt_svo_read_voxels( m_handle, xyzDev, attribsDev, stream ), "IntersectorOctreeGPU::readVoxels" );
	}
	// host-vector forms, staged through mvrt_malloc / mvrt_memcpy_*: xyz = 3 entries per voxel, attribs = 2 per voxel (empty = defaults), ops = 1 per entry (empty = all SET)
	void buildFromVoxels( const std::vector<uint32_t>& xyz, const std::vector<uint32_t>& attribs, vec3 origin, float dps, int gridRes, int buildFlags, void* stream )
	{
		const uint64_t n = xyz.size() / 3;
		Staged x( xyz.data(), xyz.size() * 4, stream ), a( attribs.empty() ? nullptr : attribs.data(), attribs.size() * 4, stream );
		buildFromVoxels( (const uint32_t*)x.p, (const uint32_t*)a.p, n, origin, dps, gridRes, buildFlags, stream );
	}
	void editVoxels( const std::vector<uint32_t>& xyz, const std::vector<uint32_t>& attribs, const std::vector<uint8_t>& ops, void* stream )
	{
		const uint64_t n = xyz.size() / 3;
		Staged x( xyz.data(), xyz.size() * 4, stream ), a( attribs.empty() ? nullptr : attribs.data(), attribs.size() * 4, stream ),
			o( ops.empty() ? nullptr : ops.data(), ops.size(), stream );
		editVoxels( (const uint32_t*)x.p, (const uint32_t*)a.p, (const uint8_t*)o.p, n, stream );
	}
	void readVoxels( std::vector<uint32_t>& xyz, std::vector<uint32_t>& attribs, void* stream ) const
	{
		mvrt_svo_info i;
		check( mvrt_svo_get_info( m_handle, &i ), "mvrt_svo_get_info" );
		Out<uint32_t> x( xyz, (uint64_t)i.numberOfVoxels * 3, stream ), a( attribs, (uint64_t)i.numberOfVoxels * 2, stream );
		readVoxels( x, a, stream );
		x.fetch( stream, true ), a.fetch( stream, true ); // (true: the one listing that asks for the copy of an empty vector too)
	}

	// the voxels of whatever octree this holds, uploaded or built, one per root-to-voxel path in ascending Morton order (mvrt_svo_walk_voxels; semantics in mvrt.h).
	// Device-pointer form: any output may be nullptr, all nullptr = the sizing call; returns the count.  A capacity below the count aborts like any failure.
	uint64_t walkVoxels( uint64_t capacity, uint32_t* xyzDev, uint32_t* vIndexDev, uint32_t* attribsDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::walkVoxels", [&]( uint64_t* n ) { return mvrt_svo_walk_voxels( m_handle, capacity, xyzDev, vIndexDev, attribsDev, n, stream ); } );
	}
	// host-vector form: xyz = 3 entries per voxel, vIndex = 1, attribs = 2
	void walkVoxels( std::vector<uint32_t>& xyz, std::vector<uint32_t>& vIndex, std::vector<uint32_t>& attribs, void* stream ) const
	{
		const uint64_t n = walkVoxels( 0, nullptr, nullptr, nullptr, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), v( vIndex, n, stream ), a( attribs, n * 2, stream );
		if( n ) walkVoxels( n, x, v, a, stream );
		fetch( stream, x, v, a );
	}
	// an uploaded octree becomes one this library built (mvrt_svo_rebuild): readVoxels / editVoxels / surface* work afterwards.  Invalidates deviceView() snapshots.
	void rebuild( int flags = 0, void* stream = nullptr )
	{
		check( mvrt_svo_rebuild( m_handle, flags, stream ), "IntersectorOctreeGPU::rebuild" );
		refresh();
	}

	// the empty cells that no path of face-neighbouring empty cells joins to the grid border, and the fill that turns them into voxels (mvrt_svo_enclosed_cells /
	// mvrt_svo_fill_enclosed; semantics in mvrt.h).  Device-pointer form: either output may be nullptr, both nullptr = the sizing call; returns the cell count.
	uint64_t enclosedCells( uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint64_t* nRegions, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::enclosedCells", [&]( uint64_t* nCells ) { return mvrt_svo_enclosed_cells( m_handle, capacity, xyzDev, regionDev, nCells, nRegions, stream ); } );
	}
	// host-vector form: xyz = 3 entries per cell in ascending Morton order, region = 1 per cell, numbered by first appearance; returns the number of regions
	uint64_t enclosedCells( std::vector<uint32_t>& xyz, std::vector<uint32_t>& region, void* stream ) const
	{
		uint64_t nRegions = 0;
		const uint64_t n = enclosedCells( 0, nullptr, nullptr, &nRegions, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), r( region, n, stream );
		if( n ) enclosedCells( n, x, r, nullptr, stream );
		fetch( stream, x, r );
		return nRegions;
	}
	// every enclosed cell becomes a voxel with fillAttrib (8 bytes VoxelAttirb, nullptr = white, no emission), as editVoxels would set it; returns the number of
	// cells filled.  0: the octree was not touched; otherwise deviceView() snapshots are invalidated.
	uint64_t fillEnclosed( const uint8_t* fillAttrib = nullptr, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::fillEnclosed", [&]( uint64_t* nFilled ) { return mvrt_svo_fill_enclosed( m_handle, fillAttrib, nFilled, stream ); } );
	}
	// the same cells with their nearest voxel, without a radius (mvrt_svo_enclosed_nearest / mvrt_svo_fill_enclosed_nearest; semantics in mvrt.h).  Device-pointer
	// form: any output may be nullptr, all nullptr = the sizing call, which computes no distance; returns the cell count.
	uint64_t enclosedNearest( uint64_t capacity, uint32_t* xyzDev, uint32_t* regionDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, uint64_t* nRegions,
							  void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::enclosedNearest", [&]( uint64_t* nCells ) {
			return mvrt_svo_enclosed_nearest( m_handle, capacity, xyzDev, regionDev, dist2Dev, nearestDev, attribsDev, nCells, nRegions, stream );
		} );
	}
	// host-vector form: xyz and region as enclosedCells gives them, dist2 = 1 entry per cell (the exact squared distance to the set, below 2^20), nearest = 1 (the
	// vIndex of the nearest voxel, the lowest on a tie), attribs = 2 (that voxel's colour and emission, alpha 255); returns the number of regions
	uint64_t enclosedNearest( std::vector<uint32_t>& xyz, std::vector<uint32_t>& region, std::vector<uint32_t>& dist2, std::vector<uint32_t>& nearest, std::vector<uint32_t>& attribs,
							  void* stream ) const
	{
		uint64_t nRegions = 0;
		const uint64_t n = enclosedNearest( 0, nullptr, nullptr, nullptr, nullptr, nullptr, &nRegions, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), r( region, n, stream ), d( dist2, n, stream ), v( nearest, n, stream ), a( attribs, n * 2, stream );
		if( n ) enclosedNearest( n, x, r, d, v, a, nullptr, stream );
		fetch( stream, x, r, d, v, a );
		return nRegions;
	}
	// every enclosed cell becomes a voxel with the colour and emission of its nearest voxel, taken on the set before the fill, as editVoxels would set it; returns
	// the number of cells filled.  0: the octree was not touched; otherwise deviceView() snapshots are invalidated.
	uint64_t fillEnclosedNearest( void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::fillEnclosedNearest", [&]( uint64_t* nFilled ) { return mvrt_svo_fill_enclosed_nearest( m_handle, nFilled, stream ); } );
	}

	// a coarser level of detail from the voxels themselves (mvrt_svo_coarse_voxels / mvrt_svo_coarsen; semantics in mvrt.h): the cells (x >> k, y >> k, z >> k),
	// k = levelsDown, that hold at least minCount voxels, each with the integer mean attribute.  Device-pointer form: any output may be nullptr, all nullptr = the
	// sizing call; returns the number of kept cells.
	uint64_t coarseVoxels( int levelsDown, uint64_t minCount, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* countDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::coarseVoxels",
						[&]( uint64_t* n ) { return mvrt_svo_coarse_voxels( m_handle, levelsDown, minCount, capacity, xyzDev, attribsDev, countDev, n, stream ); } );
	}
	// host-vector form: xyz = 3 entries per cell in ascending Morton order, attribs = 2, count = 1 (the fine voxels of the cell)
	void coarseVoxels( int levelsDown, uint64_t minCount, std::vector<uint32_t>& xyz, std::vector<uint32_t>& attribs, std::vector<uint32_t>& count, void* stream ) const
	{
		const uint64_t n = coarseVoxels( levelsDown, minCount, 0, nullptr, nullptr, nullptr, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), a( attribs, n * 2, stream ), c( count, n, stream );
		if( n ) coarseVoxels( levelsDown, minCount, n, x, a, c, stream );
		fetch( stream, x, a, c );
	}
	// dst (nullptr = this object: the in-place LOD) becomes the octree buildFromVoxels would build from that list at gridRes >> levelsDown with buildFlags, inside
	// the same bounds.  Invalidates deviceView() snapshots of dst.
	void coarsen( int levelsDown, uint64_t minCount = 1, int buildFlags = 0, IntersectorOctreeGPU* dst = nullptr, void* stream = nullptr )
	{
		IntersectorOctreeGPU* d = dst ? dst : this;
		check( mvrt_svo_coarsen( m_handle, d->m_handle, levelsDown, minCount, buildFlags, stream ), "IntersectorOctreeGPU::coarsen" );
		d->refresh();
	}

	// dilation, erosion, closing and opening of the voxel set (mvrt_svo_dilation_cells / _erosion_voxels / _dilate / _erode / _close / _open; semantics in mvrt.h),
	// element = MVRT_MORPH_FACES or MVRT_MORPH_CUBE.  Device-pointer forms of the one-step listings: any output may be nullptr, all nullptr = the sizing call; they
	// return the count.
	uint64_t dilationCells( int element, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* countDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::dilationCells", [&]( uint64_t* n ) { return mvrt_svo_dilation_cells( m_handle, element, capacity, xyzDev, attribsDev, countDev, n, stream ); } );
	}
	// host-vector form: xyz = 3 entries per cell in ascending Morton order, attribs = 2, count = 1 (the occupied neighbours of the cell)
	void dilationCells( int element, std::vector<uint32_t>& xyz, std::vector<uint32_t>& attribs, std::vector<uint32_t>& count, void* stream ) const
	{
		const uint64_t n = dilationCells( element, 0, nullptr, nullptr, nullptr, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), a( attribs, n * 2, stream ), c( count, n, stream );
		if( n ) dilationCells( element, n, x, a, c, stream );
		fetch( stream, x, a, c );
	}
	uint64_t erosionVoxels( int element, uint64_t capacity, uint32_t* vIndexDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::erosionVoxels", [&]( uint64_t* n ) { return mvrt_svo_erosion_voxels( m_handle, element, capacity, vIndexDev, n, stream ); } );
	}
	// host-vector form: the vIndex, ascending, of the voxels one erosion step removes
	void erosionVoxels( int element, std::vector<uint32_t>& vIndex, void* stream ) const
	{
		const uint64_t n = erosionVoxels( element, 0, nullptr, stream );
		Out<uint32_t> v( vIndex, n, stream );
		if( n ) erosionVoxels( element, n, v, stream );
		fetch( stream, v );
	}
	// in place, the levels built once per call.  They return the cells added (dilate), the voxels removed (erode), the net cells added (close) and the net voxels
	// removed (open).  0: the octree was not touched; otherwise deviceView() snapshots are invalidated.
	uint64_t dilate( int element = MVRT_MORPH_CUBE, int steps = 1, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::dilate", [&]( uint64_t* n ) { return mvrt_svo_dilate( m_handle, element, steps, n, stream ); } );
	}
	uint64_t erode( int element = MVRT_MORPH_CUBE, int steps = 1, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::erode", [&]( uint64_t* n ) { return mvrt_svo_erode( m_handle, element, steps, n, stream ); } );
	}
	uint64_t close( int element = MVRT_MORPH_CUBE, int steps = 1, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::close", [&]( uint64_t* n ) { return mvrt_svo_close( m_handle, element, steps, n, stream ); } );
	}
	uint64_t open( int element = MVRT_MORPH_CUBE, int steps = 1, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::open", [&]( uint64_t* n ) { return mvrt_svo_open( m_handle, element, steps, n, stream ); } );
	}

	// round offsets (mvrt_svo_distance_cells / _depth_voxels / _dilate_ball / _erode_ball / _close_ball / _open_ball; semantics in mvrt.h), radius2 = the squared
	// radius of the ball, 1..1024.  Device-pointer forms of the listings: any output may be nullptr, all nullptr = the sizing call; they return the count.
	uint64_t distanceCells( uint32_t radius2, uint64_t capacity, uint32_t* xyzDev, uint32_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::distanceCells",
						[&]( uint64_t* n ) { return mvrt_svo_distance_cells( m_handle, radius2, capacity, xyzDev, dist2Dev, nearestDev, attribsDev, n, stream ); } );
	}
	// host-vector form: xyz = 3 entries per cell in ascending Morton order, dist2 = 1 (the exact squared distance to the set), nearest = 1 (the vIndex of the
	// nearest voxel, the lowest on a tie), attribs = 2 (that voxel's colour and emission, alpha 255)
	void distanceCells( uint32_t radius2, std::vector<uint32_t>& xyz, std::vector<uint32_t>& dist2, std::vector<uint32_t>& nearest, std::vector<uint32_t>& attribs, void* stream ) const
	{
		const uint64_t n = distanceCells( radius2, 0, nullptr, nullptr, nullptr, nullptr, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), d( dist2, n, stream ), v( nearest, n, stream ), a( attribs, n * 2, stream );
		if( n ) distanceCells( radius2, n, x, d, v, a, stream );
		fetch( stream, x, d, v, a );
	}
	uint64_t depthVoxels( uint32_t radius2, uint64_t capacity, uint32_t* vIndexDev, uint32_t* depth2Dev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::depthVoxels", [&]( uint64_t* n ) { return mvrt_svo_depth_voxels( m_handle, radius2, capacity, vIndexDev, depth2Dev, n, stream ); } );
	}
	// host-vector form: the vIndex, ascending, of the voxels whose squared depth is at most radius2, and that depth
	void depthVoxels( uint32_t radius2, std::vector<uint32_t>& vIndex, std::vector<uint32_t>& depth2, void* stream ) const
	{
		const uint64_t n = depthVoxels( radius2, 0, nullptr, nullptr, stream );
		Out<uint32_t> v( vIndex, n, stream ), d( depth2, n, stream );
		if( n ) depthVoxels( radius2, n, v, d, stream );
		fetch( stream, v, d );
	}
	// in place, one ball per call, the levels built once.  They return the cells added (dilateBall), the voxels removed (erodeBall), the net cells added (closeBall)
	// and the net voxels removed (openBall).  0: the octree was not touched; otherwise deviceView() snapshots are invalidated.
	uint64_t dilateBall( uint32_t radius2, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::dilateBall", [&]( uint64_t* n ) { return mvrt_svo_dilate_ball( m_handle, radius2, n, stream ); } );
	}
	uint64_t erodeBall( uint32_t radius2, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::erodeBall", [&]( uint64_t* n ) { return mvrt_svo_erode_ball( m_handle, radius2, n, stream ); } );
	}
	uint64_t closeBall( uint32_t radius2, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::closeBall", [&]( uint64_t* n ) { return mvrt_svo_close_ball( m_handle, radius2, n, stream ); } );
	}
	uint64_t openBall( uint32_t radius2, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::openBall", [&]( uint64_t* n ) { return mvrt_svo_open_ball( m_handle, radius2, n, stream ); } );
	}

	// connected components of the voxel set (mvrt_svo_components / mvrt_svo_keep_components; semantics in mvrt.h), element = MVRT_MORPH_FACES (6-connected) or
	// MVRT_MORPH_CUBE (26-connected).  Device-pointer form: labelDev holds numberOfVoxels entries, the others componentCapacity components (boxDev 6 each); any
	// output may be nullptr, all nullptr = the sizing call.  Returns the number of components; *largest (may be nullptr) = the size of the largest.
	uint64_t components( int element, uint32_t* labelDev, uint64_t componentCapacity, uint32_t* sizeDev, uint32_t* firstDev, uint32_t* boxDev, uint64_t* largest, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::components",
						[&]( uint64_t* n ) { return mvrt_svo_components( m_handle, element, labelDev, componentCapacity, sizeDev, firstDev, boxDev, n, largest, stream ); } );
	}
	// host-vector form: label = one entry per voxel in vIndex order, numbered by first appearance; per component size = 1 entry, first = 1 (its lowest vIndex),
	// box = 6 (min x, y, z, max x, y, z)
	void components( int element, std::vector<uint32_t>& label, std::vector<uint32_t>& size, std::vector<uint32_t>& first, std::vector<uint32_t>& box, void* stream ) const
	{
		const uint64_t n = components( element, nullptr, 0, nullptr, nullptr, nullptr, nullptr, stream );
		Out<uint32_t> l( label, m_numberOfVoxels, stream ), s( size, n, stream ), f( first, n, stream ), b( box, n * 6, stream );
		components( element, l, n, s, f, b, nullptr, stream ); // (made at n == 0 too, unlike the listings above)
		fetch( stream, l, s, f, b );
	}
	// in place: keeps the components of at least minVoxels voxels and, where keepLargest != 0, only the keepLargest largest of them (a tie goes to the component
	// that appears first).  Returns the voxels removed; *keptComponents (may be nullptr) = the components kept.  0: the octree was not touched; otherwise
	// deviceView() snapshots are invalidated.
	uint64_t keepComponents( int element = MVRT_MORPH_CUBE, uint64_t minVoxels = 1, uint32_t keepLargest = 0, uint64_t* keptComponents = nullptr, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::keepComponents",
					   [&]( uint64_t* n ) { return mvrt_svo_keep_components( m_handle, element, minVoxels, keepLargest, n, keptComponents, stream ); } );
	}

	// boolean operations with a second voxel set moved by an integer cell offset (mvrt_svo_combine_voxels / mvrt_svo_combine; semantics in mvrt.h): op = COMBINE_*,
	// offset = 3 ints or nullptr (zero), flags = 0 or COMBINE_ATTRIB_B.  Device-pointer form of the listing: any output may be nullptr, all nullptr = the sizing
	// call.  Returns the number of voxels; *overlap and *clipped (either may be nullptr) = the voxels in both sets and the voxels of b moved out of the grid.
	enum
	{
		COMBINE_UNION = MVRT_COMBINE_UNION,
		COMBINE_INTERSECTION = MVRT_COMBINE_INTERSECTION,
		COMBINE_DIFFERENCE = MVRT_COMBINE_DIFFERENCE,
		COMBINE_XOR = MVRT_COMBINE_XOR,
		COMBINE_ATTRIB_B = MVRT_COMBINE_ATTRIB_B
	};
	uint64_t combineVoxels( const IntersectorOctreeGPU& b, int op, const int32_t* offset, uint32_t flags, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev,
							uint8_t* sourceDev, uint64_t* overlap, uint64_t* clipped, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::combineVoxels", [&]( uint64_t* n ) {
			return mvrt_svo_combine_voxels( m_handle, b.m_handle, op, offset, flags, capacity, xyzDev, attribsDev, sourceDev, n, overlap, clipped, stream );
		} );
	}
	// host-vector form: xyz = 3 entries per voxel in ascending Morton order, attribs = 2, source = 1 byte (1 = this set only, 2 = b only, 3 = both)
	void combineVoxels( const IntersectorOctreeGPU& b, int op, const int32_t* offset, uint32_t flags, std::vector<uint32_t>& xyz, std::vector<uint32_t>& attribs,
						std::vector<uint8_t>& source, uint64_t* overlap, uint64_t* clipped, void* stream ) const
	{
		const uint64_t n = combineVoxels( b, op, offset, flags, 0, nullptr, nullptr, nullptr, overlap, clipped, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), a( attribs, n * 2, stream );
		Out<uint8_t> s( source, n, stream );
		if( n ) combineVoxels( b, op, offset, flags, n, x, a, s, nullptr, nullptr, stream );
		fetch( stream, x, a, s );
	}
	// in place: this octree becomes the result, exactly as the edit with the added voxels as MVRT_VOXEL_SET and the dropped ones as MVRT_VOXEL_REMOVE leaves it; b
	// may be this object.  Returns the voxels added; *removed and *clipped may be nullptr.  A call that changes nothing does not touch the octree; otherwise
	// deviceView() snapshots are invalidated.
	uint64_t combine( const IntersectorOctreeGPU& b, int op, const int32_t* offset = nullptr, uint32_t flags = 0, uint64_t* removed = nullptr, uint64_t* clipped = nullptr,
					  void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::combine", [&]( uint64_t* n ) { return mvrt_svo_combine( m_handle, b.m_handle, op, offset, flags, n, removed, clipped, stream ); } );
	}

	// the nearest voxel of arbitrary lattice points, the distance to a second voxel set and the recolouring from it (mvrt_svo_nearest_voxels / _nearest_between /
	// _transfer_attributes; semantics in mvrt.h).  maxDist2 = NO_LIMIT: no limit; a query beyond the limit reports dist2 NO_LIMIT, nearest 0xFFFFFFFF, attribs 0.
	// Device-pointer form: n queries of 3 int32 each, any output may be nullptr
	static constexpr uint64_t NO_LIMIT = ~0ull;
	enum
	{
		TRANSFER_COLOUR = MVRT_TRANSFER_COLOUR,
		TRANSFER_EMISSION = MVRT_TRANSFER_EMISSION
	};
	void nearestVoxels( uint64_t n, const int32_t* queryDev, uint64_t maxDist2, uint64_t* dist2Dev, uint32_t* nearestDev, uint32_t* attribsDev, void* stream ) const
	{
		check( mvrt_svo_nearest_voxels( m_handle, n, queryDev, maxDist2, dist2Dev, nearestDev, attribsDev, stream ), "IntersectorOctreeGPU::nearestVoxels" );
	}
	// host-vector form: query = 3 entries per point; dist2 and nearest = 1 entry per point in the caller's order, attribs = 2
	void nearestVoxels( const std::vector<int32_t>& query, uint64_t maxDist2, std::vector<uint64_t>& dist2, std::vector<uint32_t>& nearest, std::vector<uint32_t>& attribs,
						void* stream ) const
	{
		const uint64_t n = query.size() / 3;
		nearestVoxels( 0, nullptr, maxDist2, nullptr, nullptr, nullptr, stream ); // (what the handle decides is refused before anything is allocated)
		Staged q( query.data(), n * 12, stream );
		Out<uint64_t> d( dist2, n, stream );
		Out<uint32_t> v( nearest, n, stream ), a( attribs, n * 2, stream );
		if( n ) nearestVoxels( n, (const int32_t*)q.p, maxDist2, d, v, a, stream );
		fetch( stream, d, v, a );
	}
	// every voxel v of this set, in vIndex order, asked as v - offset (3 ints or nullptr = zero) in b; b may be this object
	struct Between
	{
		uint64_t n = 0, maxDist2 = 0, nZero = 0, nBeyond = 0; // this set's voxels, the largest dist2 within the limit, the voxels at distance 0, those beyond the limit
		uint32_t farthest = 0;								  // the lowest vIndex of this set that attains maxDist2
	};
	// device-pointer form: either array may be nullptr, both nullptr = the summary call
	Between nearestBetween( const IntersectorOctreeGPU& b, const int32_t* offset, uint64_t maxDist2, uint64_t capacity, uint64_t* dist2Dev, uint32_t* nearestDev, void* stream ) const
	{
		Between r;
		check( mvrt_svo_nearest_between( m_handle, b.m_handle, offset, maxDist2, capacity, dist2Dev, nearestDev, &r.n, &r.maxDist2, &r.farthest, &r.nZero, &r.nBeyond, stream ),
			   "IntersectorOctreeGPU::nearestBetween" );
		return r;
	}
	Between nearestBetween( const IntersectorOctreeGPU& b, const int32_t* offset, uint64_t maxDist2, std::vector<uint64_t>& dist2, std::vector<uint32_t>& nearest, void* stream ) const
	{
		mvrt_svo_info i;
		check( mvrt_svo_get_info( m_handle, &i ), "IntersectorOctreeGPU::nearestBetween" );
		const uint64_t n = i.numberOfVoxels;
		if( !n ) return nearestBetween( b, offset, maxDist2, 0, nullptr, nullptr, stream ); // (an empty handle: the call refuses it)
		Out<uint64_t> d( dist2, n, stream );
		Out<uint32_t> v( nearest, n, stream );
		const Between r = nearestBetween( b, offset, maxDist2, n, d, v, stream );
		fetch( stream, d, v );
		return r;
	}
	// in place: every voxel with a voxel of src within maxDist2 takes the words `flags` names (TRANSFER_COLOUR | TRANSFER_EMISSION) of the nearest one, exactly as the
	// edit with MVRT_VOXEL_SET stores them; src may be this object.  Returns the voxels whose bytes changed; *beyond may be nullptr.  A call that changes no byte
	// does not touch the octree; otherwise the attributes are written in place, the nodes stay, and hasEmission is recomputed (a deviceView() snapshot keeps the old flag)
	uint64_t transferAttributes( const IntersectorOctreeGPU& src, const int32_t* offset = nullptr, uint64_t maxDist2 = NO_LIMIT, uint32_t flags = TRANSFER_COLOUR | TRANSFER_EMISSION,
								 uint64_t* beyond = nullptr, void* stream = nullptr )
	{
		return edited( "IntersectorOctreeGPU::transferAttributes",
					   [&]( uint64_t* n ) { return mvrt_svo_transfer_attributes( m_handle, src.m_handle, offset, maxDist2, flags, n, beyond, stream ); } );
	}

	// the voxel set resampled onto a grid of dstGridRes cells per axis under an affine map (mvrt_svo_resample_voxels / mvrt_svo_resample; semantics in mvrt.h): xf is
	// the INVERSE map, destination cells to source cells, in fixed point; cellTransformFromWorld makes it from a world matrix and two lattices.  Device-pointer form
	// of the listing: any output may be nullptr, all nullptr = the sizing call.  Returns the number of voxels.
	static mvrt_cell_transform cellTransformFromWorld( const double world[12], vec3 srcLower, float srcDps, vec3 dstLower, float dstDps )
	{
		mvrt_cell_transform xf;
		const float sl[3] = { srcLower.x, srcLower.y, srcLower.z }, dl[3] = { dstLower.x, dstLower.y, dstLower.z };
		check( mvrt_cell_transform_from_world( world, sl, srcDps, dl, dstDps, &xf ), "IntersectorOctreeGPU::cellTransformFromWorld" );
		return xf;
	}
	uint64_t resampleVoxels( const mvrt_cell_transform& xf, int dstGridRes, uint64_t capacity, uint32_t* xyzDev, uint32_t* attribsDev, uint32_t* sourceDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::resampleVoxels",
						[&]( uint64_t* n ) { return mvrt_svo_resample_voxels( m_handle, &xf, dstGridRes, capacity, xyzDev, attribsDev, sourceDev, n, stream ); } );
	}
	// host-vector form: xyz = 3 entries per voxel in ascending Morton order of the destination grid, attribs = 2, source = 1 (the vIndex the voxel comes from)
	void resampleVoxels( const mvrt_cell_transform& xf, int dstGridRes, std::vector<uint32_t>& xyz, std::vector<uint32_t>& attribs, std::vector<uint32_t>& source, void* stream ) const
	{
		const uint64_t n = resampleVoxels( xf, dstGridRes, 0, nullptr, nullptr, nullptr, stream );
		Out<uint32_t> x( xyz, n * 3, stream ), a( attribs, n * 2, stream ), s( source, n, stream );
		if( n ) resampleVoxels( xf, dstGridRes, n, x, a, s, stream );
		fetch( stream, x, a, s );
	}
	// dst (nullptr = this object) becomes the octree buildFromVoxels would build from that list with dstOrigin, dstDps, dstGridRes and buildFlags.  Returns the voxels
	// of the result; an empty result aborts like any failure.  Invalidates deviceView() snapshots of dst.
	uint64_t resample( const mvrt_cell_transform& xf, vec3 dstOrigin, float dstDps, int dstGridRes, int buildFlags = 0, IntersectorOctreeGPU* dst = nullptr, void* stream = nullptr )
	{
		IntersectorOctreeGPU* d = dst ? dst : this;
		const float o[3] = { dstOrigin.x, dstOrigin.y, dstOrigin.z };
		return d->edited( "IntersectorOctreeGPU::resample", // (d->: it is dst that is refreshed)
						  [&]( uint64_t* n ) { return mvrt_svo_resample( m_handle, d->m_handle, &xf, o, dstDps, dstGridRes, buildFlags, n, stream ); } );
	}

	// the exposed faces of the voxel set as quads (mvrt_svo_surface_masks / _quads / _mesh; semantics in mvrt.h; the reference's Save As Mesh, voxMesh.cpp:111-219).
	// Device-pointer forms: any output may be nullptr, all nullptr = the sizing call; they return the counts.  A capacity below the count aborts like any failure.
	uint64_t surfaceMasks( uint8_t* masksDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::surfaceMasks", [&]( uint64_t* nFaces ) { return mvrt_svo_surface_masks( m_handle, masksDev, nFaces, stream ); } );
	}
	uint64_t surfaceQuads( uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::surfaceQuads",
						[&]( uint64_t* nFaces ) { return mvrt_svo_surface_quads( m_handle, faceCapacity, faceVoxelDev, faceDirDev, positionsDev, nFaces, stream ); } );
	}
	void surfaceMesh( uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFaces,
					  uint64_t* nVertices, void* stream ) const
	{
		check( mvrt_svo_surface_mesh( m_handle, faceCapacity, vertexCapacity, faceVoxelDev, faceDirDev, indicesDev, verticesDev, nFaces, nVertices, stream ),
			   "IntersectorOctreeGPU::surfaceMesh" );
	}
	// host-vector forms: sized here (the sizing call, then the real one), staged through mvrt_malloc / mvrt_memcpy_d2h
	uint64_t surfaceMasks( std::vector<uint8_t>& masks, void* stream ) const
	{
		Out<uint8_t> m( masks, m_numberOfVoxels, stream );
		const uint64_t nFaces = surfaceMasks( m, stream );
		fetch( stream, m );
		return nFaces;
	}
	// (the host-vector forms of quads, mesh, merged and ao and their *Masked twins are one private template each, below: quadsToHost, meshToHost, mergedToHost,
	// aoToHost; `a...` = the capacities, outputs and counters as the template passes them to the device-pointer form)
	void surfaceQuads( std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, std::vector<float>& positions /* 12 per face */, void* stream ) const
	{
		quadsToHost( [&]( const auto&... a ) { return surfaceQuads( a..., stream ); }, faceVoxel, faceDir, positions, stream );
	}
	void surfaceMesh( std::vector<float>& vertices /* 3 per vertex */, std::vector<uint32_t>& indices /* 4 per face */, std::vector<uint32_t>& faceVoxel,
					  std::vector<uint8_t>& faceDir, void* stream ) const
	{
		meshToHost( [&]( const auto&... a ) { surfaceMesh( a..., stream ); }, vertices, indices, faceVoxel, faceDir, stream );
	}

	// the same surface with coplanar faces merged into rectangles (mvrt_svo_surface_merged; the rule is in mvrt.h).  flags: MVRT_SURFACE_MERGE_ANY_ATTRIBUTE |
	// MVRT_SURFACE_MERGE_WELD; indicesDev / verticesDev need the weld flag.  Device-pointer form: any output may be nullptr, all nullptr = the sizing call.
	void surfaceMerged( uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev, uint8_t* rectDirDev, uint32_t* rectSizeDev, float* positionsDev,
						uint32_t* indicesDev, float* verticesDev, uint64_t* nFaces, uint64_t* nRects, uint64_t* nVertices, void* stream ) const
	{
		check( mvrt_svo_surface_merged( m_handle, flags, rectCapacity, vertexCapacity, rectVoxelDev, rectDirDev, rectSizeDev, positionsDev, indicesDev, verticesDev, nFaces, nRects,
										nVertices, stream ),
			   "IntersectorOctreeGPU::surfaceMerged" );
	}
	// host-vector form.  With the weld flag: shared vertices and 4 indices per rectangle, like surfaceMesh.  Without it: `vertices` holds the 4 corners of every
	// rectangle (12 floats each) and `indices` stays empty.  Returns nFaces, the number of voxel faces the rectangles cover.
	uint64_t surfaceMerged( uint32_t flags, std::vector<float>& vertices, std::vector<uint32_t>& indices, std::vector<uint32_t>& rectVoxel, std::vector<uint8_t>& rectDir,
							std::vector<uint32_t>& rectSize /* 2 per rectangle */, void* stream ) const
	{
		return mergedToHost( [&]( const auto&... a ) { surfaceMerged( flags, a..., stream ); }, flags, vertices, indices, rectVoxel, rectDir, rectSize, stream );
	}

	// exterior-only masks and the three extraction calls on face masks the caller supplies (mvrt_svo_surface_exterior_masks / mvrt_svo_surface_*_masked; semantics in
	// mvrt.h): the masks of surfaceMasks without the bits that look into an enclosed cell, the octree untouched; and surfaceQuads / surfaceMesh / surfaceMerged
	// whose faces are the set bits 0..5 of numberOfVoxels mask bytes, taken as given.  Device-pointer forms; masksDev of surfaceExteriorMasks may be nullptr
	// (counts only); returns the exterior faces, *nHidden = the faces of surfaceMasks minus those
	uint64_t surfaceExteriorMasks( uint8_t* masksDev, uint64_t* nHidden, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::surfaceExteriorMasks",
						[&]( uint64_t* nFaces ) { return mvrt_svo_surface_exterior_masks( m_handle, masksDev, nFaces, nHidden, stream ); } );
	}
	uint64_t surfaceQuadsMasked( const uint8_t* masksDev, uint64_t faceCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, float* positionsDev, void* stream ) const
	{
		return counted( "IntersectorOctreeGPU::surfaceQuadsMasked", [&]( uint64_t* nFaces ) {
			return mvrt_svo_surface_quads_masked( m_handle, masksDev, faceCapacity, faceVoxelDev, faceDirDev, positionsDev, nFaces, stream );
		} );
	}
	void surfaceMeshMasked( const uint8_t* masksDev, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev, uint32_t* indicesDev,
							float* verticesDev, uint64_t* nFaces, uint64_t* nVertices, void* stream ) const
	{
		check( mvrt_svo_surface_mesh_masked( m_handle, masksDev, faceCapacity, vertexCapacity, faceVoxelDev, faceDirDev, indicesDev, verticesDev, nFaces, nVertices, stream ),
			   "IntersectorOctreeGPU::surfaceMeshMasked" );
	}
	void surfaceMergedMasked( const uint8_t* masksDev, uint32_t flags, uint64_t rectCapacity, uint64_t vertexCapacity, uint32_t* rectVoxelDev, uint8_t* rectDirDev,
							  uint32_t* rectSizeDev, float* positionsDev, uint32_t* indicesDev, float* verticesDev, uint64_t* nFaces, uint64_t* nRects, uint64_t* nVertices,
							  void* stream ) const
	{
		check( mvrt_svo_surface_merged_masked( m_handle, masksDev, flags, rectCapacity, vertexCapacity, rectVoxelDev, rectDirDev, rectSizeDev, positionsDev, indicesDev, verticesDev,
											   nFaces, nRects, nVertices, stream ),
			   "IntersectorOctreeGPU::surfaceMergedMasked" );
	}
	// host-vector forms, like their namesakes; `masks` holds numberOfVoxels bytes
	uint64_t surfaceExteriorMasks( std::vector<uint8_t>& masks, uint64_t* nHidden, void* stream ) const
	{
		Out<uint8_t> m( masks, m_numberOfVoxels, stream );
		const uint64_t nFaces = surfaceExteriorMasks( m, nHidden, stream );
		fetch( stream, m );
		return nFaces;
	}
	void surfaceQuadsMasked( const std::vector<uint8_t>& masks, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, std::vector<float>& positions /* 12 per face */,
							 void* stream ) const
	{
		Staged m( masks.data(), masks.size(), stream );
		quadsToHost( [&]( const auto&... a ) { return surfaceQuadsMasked( (const uint8_t*)m.p, a..., stream ); }, faceVoxel, faceDir, positions, stream );
	}
	void surfaceMeshMasked( const std::vector<uint8_t>& masks, std::vector<float>& vertices /* 3 per vertex */, std::vector<uint32_t>& indices /* 4 per face */,
							std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, void* stream ) const
	{
		Staged m( masks.data(), masks.size(), stream );
		meshToHost( [&]( const auto&... a ) { surfaceMeshMasked( (const uint8_t*)m.p, a..., stream ); }, vertices, indices, faceVoxel, faceDir, stream );
	}
	uint64_t surfaceMergedMasked( const std::vector<uint8_t>& masks, uint32_t flags, std::vector<float>& vertices, std::vector<uint32_t>& indices, std::vector<uint32_t>& rectVoxel,
								  std::vector<uint8_t>& rectDir, std::vector<uint32_t>& rectSize /* 2 per rectangle */, void* stream ) const
	{
		Staged m( masks.data(), masks.size(), stream );
		return mergedToHost( [&]( const auto&... a ) { surfaceMergedMasked( (const uint8_t*)m.p, flags, a..., stream ); }, flags, vertices, indices, rectVoxel, rectDir, rectSize,
							 stream );
	}
	// the faces of surfaceQuadsMasked with their occlusion (surfaceAo below takes any face list)
	void surfaceAoMasked( const std::vector<uint8_t>& masks, int samples, float radius, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, std::vector<uint16_t>& open,
						  void* stream ) const
	{
		Staged m( masks.data(), masks.size(), stream );
		aoToHost( [&]( const auto&... a ) { return surfaceQuadsMasked( (const uint8_t*)m.p, a..., stream ); }, samples, radius, faceVoxel, faceDir, open, stream );
	}

	// the welded mesh smoothed by constrained surface nets (mvrt_svo_surface_smooth; the rule is in mvrt.h): the faces, indices and vertex order of surfaceMesh (of
	// surfaceMeshMasked for masksDev != nullptr), the vertices relaxed inside a box around their lattice corners.  params nullptr = smoothDefaultParams().
	// Device-pointer form: any output may be nullptr, all nullptr = the sizing call, which runs no iteration; displacementsDev (3 int32 per vertex, steps of
	// 1 / 256 cell) and neighboursDev (1 byte per vertex) follow vertexCapacity.  *clamped: the axes an iteration held at the limit, over all iterations
	static mvrt_smooth_params smoothDefaultParams()
	{
		mvrt_smooth_params p;
		check( mvrt_smooth_default_params( &p ), "IntersectorOctreeGPU::smoothDefaultParams" );
		return p;
	}
	void surfaceSmooth( const uint8_t* masksDev, const mvrt_smooth_params* params, uint64_t faceCapacity, uint64_t vertexCapacity, uint32_t* faceVoxelDev, uint8_t* faceDirDev,
						uint32_t* indicesDev, float* verticesDev, int32_t* displacementsDev, uint8_t* neighboursDev, uint64_t* nFaces, uint64_t* nVertices, uint64_t* clamped,
						void* stream ) const
	{
		check( mvrt_svo_surface_smooth( m_handle, masksDev, params, faceCapacity, vertexCapacity, faceVoxelDev, faceDirDev, indicesDev, verticesDev, displacementsDev, neighboursDev,
										nFaces, nVertices, clamped, stream ),
			   "IntersectorOctreeGPU::surfaceSmooth" );
	}
	// host-vector forms, like surfaceMesh; returns the clamped count.  `masks`: numberOfVoxels bytes, the faces to smooth (surfaceMeshMasked)
	uint64_t surfaceSmooth( const mvrt_smooth_params& params, std::vector<float>& vertices /* 3 per vertex */, std::vector<uint32_t>& indices /* 4 per face */,
							std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, void* stream ) const
	{
		return smoothToHost( nullptr, params, vertices, indices, faceVoxel, faceDir, stream );
	}
	uint64_t surfaceSmooth( const std::vector<uint8_t>& masks, const mvrt_smooth_params& params, std::vector<float>& vertices /* 3 per vertex */,
							std::vector<uint32_t>& indices /* 4 per face */, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, void* stream ) const
	{
		Staged m( masks.data(), masks.size(), stream );
		return smoothToHost( (const uint8_t*)m.p, params, vertices, indices, faceVoxel, faceDir, stream );
	}

	// batch form of the device method intersect() (:243-251): SoA device arrays
	void intersect( uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz, const uint8_t* isShadowRay, float* t,
					int32_t* nMajor, uint32_t* vIndex, void* stream ) const
	{
		check( mvrt_trace_batch( m_handle, n, rox, roy, roz, rdx, rdy, rdz, isShadowRay, t, nMajor, vIndex, nullptr, stream ), "IntersectorOctreeGPU::intersect" );
	}
	// the same rays with a distance limit per ray (mvrt_trace_batch_range): the hit of intersect() where its t <= tMax[i], else a miss; descents may be nullptr
	void intersectRange( uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz, const uint8_t* isShadowRay,
						 const float* tMax, float* t, int32_t* nMajor, uint32_t* vIndex, uint32_t* descents, void* stream ) const
	{
		check( mvrt_trace_batch_range( m_handle, n, rox, roy, roz, rdx, rdy, rdz, isShadowRay, tMax, t, nMajor, vIndex, descents, stream ), "IntersectorOctreeGPU::intersectRange" );
	}
	// per-face ambient occlusion (mvrt_svo_surface_ao): open[f] of `samples` rays leave face f unoccluded within `radius`.  Device-pointer form
	void surfaceAo( uint64_t nFaces, const uint32_t* faceVoxelDev, const uint8_t* faceDirDev, int samples, float radius, uint16_t* openDev, void* stream ) const
	{
		check( mvrt_svo_surface_ao( m_handle, nFaces, faceVoxelDev, faceDirDev, samples, radius, openDev, stream ), "IntersectorOctreeGPU::surfaceAo" );
	}
	// host-vector form: the faces of surfaceQuads with their occlusion
	void surfaceAo( int samples, float radius, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, std::vector<uint16_t>& open, void* stream ) const
	{
		aoToHost( [&]( const auto&... a ) { return surfaceQuads( a..., stream ); }, samples, radius, faceVoxel, faceDir, open, stream );
	}
	// the table of occlusion ray directions (mvrt_ao_directions): 6 * samples * 3 floats, host only
	static std::vector<float> aoDirections( int samples )
	{
		std::vector<float> dirs( samples > 0 ? (size_t)6 * samples * 3 : 0 );
		check( mvrt_ao_directions( samples, dirs.data() ), "IntersectorOctreeGPU::aoDirections" );
		return dirs;
	}
	bool hasEmission() const { return m_hasEmission != 0; } // :261-264

	// the by-value struct a user kernel takes (include/mvrt/device.hpp: mvrt::DeviceOctree).  emissionScale is this object's m_emissionScale, so
	// assigning that member takes effect in kernels written on the device API.  Invalidated by the next build / upload / cleanUp (a snapshot).
	mvrt_device_octree deviceView() const
	{
		mvrt_device_octree v;
		check( mvrt_svo_device_view( m_handle, &v ), "IntersectorOctreeGPU::deviceView" );
		v.emissionScale = m_emissionScale;
		return v;
	}

	// level of detail per ray (mvrt_svo_lod_prepare / _release / _bytes / _view, mvrt_trace_batch_cone, mvrt_render_primary_lod; semantics in mvrt.h).  The pyramid
	// is dropped by whatever changes the voxels; lodView() is a snapshot like deviceView()
	void lodPrepare( void* stream = nullptr ) { check( mvrt_svo_lod_prepare( m_handle, stream ), "IntersectorOctreeGPU::lodPrepare" ); }
	void lodRelease() { check( mvrt_svo_lod_release( m_handle ), "IntersectorOctreeGPU::lodRelease" ); }
	uint64_t lodBytes() const { return mvrt_svo_lod_bytes( m_handle ); }
	mvrt_device_lod lodView() const
	{
		mvrt_device_lod v;
		check( mvrt_svo_lod_view( m_handle, &v ), "IntersectorOctreeGPU::lodView" );
		return v;
	}
	// cone-limited rays on device arrays: every output but t may be nullptr; index and attrib (2 words per ray) need lodPrepare()
	void intersectCone( uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz, const float* coneA, const float* coneB,
						float* t, int32_t* nMajor, uint32_t* level, uint64_t* cellCode, uint32_t* index, uint32_t* attrib, uint32_t* descents, void* stream ) const
	{
		check( mvrt_trace_batch_cone( m_handle, n, rox, roy, roz, rdx, rdy, rdz, coneA, coneB, t, nMajor, level, cellCode, index, attrib, descents, stream ),
			   "IntersectorOctreeGPU::intersectCone" );
	}
	void renderLod( const float camera[15], int width, int height, float lodScale, bool showVertexColor, uint8_t* rgbaDev, float* tDev, int32_t* nMajorDev, uint32_t* levelDev,
					uint32_t* descentsDev, void* stream ) const
	{
		check( mvrt_render_primary_lod( m_handle, camera, width, height, lodScale, showVertexColor ? 1 : 0, rgbaDev, tDev, nMajorDev, levelDev, descentsDev, stream ),
			   "IntersectorOctreeGPU::renderLod" );
	}

	mvrt_svo* handle() const { return m_handle; }

	// re-bind to a handle owned by someone else (PathTracer::m_intersectorOctreeGPU is a VALUE member in the reference, PathTracer.hpp:18)
	void attach( mvrt_svo* borrowed )
	{
		if( m_owned && m_handle ) mvrt_svo_destroy( m_handle );
		m_handle = borrowed;
		m_owned = false;
		refresh();
	}

	// reference public members (:265-274), refreshed after build/upload
	const void* m_vAttributeBuffer = nullptr; // device: VoxelAttirb[m_numberOfVoxels]
	const void* m_nodeBuffer = nullptr;		  // device: 64-byte node lines (see mvrt.h; mvrt_svo_download gives the reference's 68-byte nodes)
	uint32_t m_numberOfNodes = 0;
	uint32_t m_numberOfVoxels = 0;
	vec3 m_lower = { 0, 0, 0 };
	vec3 m_upper = { 0, 0, 0 };
	float m_dps = 0.0f;
	float m_emissionScale = 7.5f;
	uint32_t m_hasEmission = 0;

	void refresh()
	{
		mvrt_svo_info i;
		if( !m_handle || mvrt_svo_get_info( m_handle, &i ) != 0 ) return;
		m_vAttributeBuffer = mvrt_svo_attribute_buffer_dev( m_handle );
		m_nodeBuffer = mvrt_svo_node_buffer_dev( m_handle );
		m_numberOfNodes = i.numberOfNodes;
		m_numberOfVoxels = i.numberOfVoxels;
		m_lower = { i.lower[0], i.lower[1], i.lower[2] };
		m_upper = { i.upper[0], i.upper[1], i.upper[2] };
		m_dps = i.dps;
		m_emissionScale = i.emissionScale;
		m_hasEmission = i.hasEmission;
	}

private:
	struct Staged // a device copy of host data (or uninitialised device memory when src is null and bytes != 0); no allocation for an absent array
	{
		void* p = nullptr;
		Staged( const void* src, uint64_t bytes, void* stream )
		{
			if( !bytes ) return;
			check( mvrt_malloc( &p, bytes ), "mvrt_malloc" );
			if( src ) check( mvrt_memcpy_h2d( p, src, bytes, stream ), "mvrt_memcpy_h2d" );
		}
		~Staged() { mvrt_free( p ); }
		Staged( const Staged& ) = delete;
		void operator=( const Staged& ) = delete;
	};
	// one output of a host-vector form: the caller's vector, resized to `count` entries, tied to its uninitialised staging block on the device (none for count 0).
	// It converts to the T* the device-pointer forms take.  A listing declares its outputs once, in allocation order, and copies them back with fetch(): not in
	// a destructor, since check() aborts and an abort while unwinding would hide the first error.
	template <class T> struct Out
	{
		std::vector<T>& host;
		Staged dev;
		Out( std::vector<T>& h, uint64_t count, void* stream ) : host( ( h.resize( count ), h ) ), dev( nullptr, count * sizeof( T ), stream ) {}
		operator T*() const { return (T*)dev.p; }
		void fetch( void* stream, bool copyEmpty = false ) const // device -> host vector of the same size (nothing for an empty one)
		{
			if( copyEmpty || !host.empty() ) check( mvrt_memcpy_d2h( host.data(), dev.p, host.size() * sizeof( T ), stream ), "mvrt_memcpy_d2h" );
		}
	};
	template <class... O> static void fetch( void* stream, const O&... outs ) { ( outs.fetch( stream ), ... ); } // in the order given
	// a call that reports its first count through the pointer it is handed: checked under `label`; edited(): an in-place operation, the members refreshed after it
	template <class Call> static uint64_t counted( const char* label, Call call )
	{
		uint64_t n = 0;
		check( call( &n ), label );
		return n;
	}
	template <class Call> uint64_t edited( const char* label, Call call )
	{
		const uint64_t n = counted( label, call );
		refresh();
		return n;
	}
	// the host-vector forms of the surface listings, `quads` / `mesh` / `merged` = the device-pointer form without its stream (surfaceQuads or surfaceQuadsMasked
	// on staged masks, ...).  Unlike the voxel listings they make the filling call at a count of 0 too.
	template <class Quads> void quadsToHost( Quads quads, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, std::vector<float>& positions, void* stream ) const
	{
		const uint64_t n = quads( 0, nullptr, nullptr, nullptr );
		Out<uint32_t> v( faceVoxel, n, stream );
		Out<uint8_t> d( faceDir, n, stream );
		Out<float> p( positions, n * 12, stream );
		quads( n, v, d, p );
		fetch( stream, v, d, p );
	}
	template <class Mesh>
	void meshToHost( Mesh mesh, std::vector<float>& vertices, std::vector<uint32_t>& indices, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, void* stream ) const
	{
		uint64_t nf = 0, nv = 0;
		mesh( 0, 0, nullptr, nullptr, nullptr, nullptr, &nf, &nv );
		Out<float> x( vertices, nv * 3, stream );
		Out<uint32_t> i( indices, nf * 4, stream ), v( faceVoxel, nf, stream );
		Out<uint8_t> d( faceDir, nf, stream );
		mesh( nf, nv, v, d, i, x, &nf, &nv );
		fetch( stream, x, i, v, d );
	}
	uint64_t smoothToHost( const uint8_t* masksDev, const mvrt_smooth_params& params, std::vector<float>& vertices, std::vector<uint32_t>& indices, std::vector<uint32_t>& faceVoxel,
						   std::vector<uint8_t>& faceDir, void* stream ) const
	{
		uint64_t clamped = 0;
		meshToHost( [&]( uint64_t fc, uint64_t vc, uint32_t* v, uint8_t* d, uint32_t* i, float* x, uint64_t* nf, uint64_t* nv ) {
			surfaceSmooth( masksDev, &params, fc, vc, v, d, i, x, nullptr, nullptr, nf, nv, &clamped, stream );
		}, vertices, indices, faceVoxel, faceDir, stream );
		return clamped;
	}
	template <class Merged>
	uint64_t mergedToHost( Merged merged, uint32_t flags, std::vector<float>& vertices, std::vector<uint32_t>& indices, std::vector<uint32_t>& rectVoxel, std::vector<uint8_t>& rectDir,
						   std::vector<uint32_t>& rectSize, void* stream ) const
	{
		const bool weld = ( flags & MVRT_SURFACE_MERGE_WELD ) != 0;
		uint64_t nf = 0, nr = 0, nv = 0;
		merged( 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nf, &nr, &nv );
		Out<float> x( vertices, ( weld ? nv : nr * 4 ) * 3, stream ); // welded: the shared vertices; else the positions, 4 corners per rectangle
		Out<uint32_t> i( indices, weld ? nr * 4 : 0, stream ), v( rectVoxel, nr, stream );
		Out<uint8_t> d( rectDir, nr, stream );
		Out<uint32_t> s( rectSize, nr * 2, stream );
		merged( nr, nv, v, d, s, weld ? nullptr : (float*)x, weld ? (uint32_t*)i : nullptr, weld ? (float*)x : nullptr, &nf, &nr, &nv );
		fetch( stream, x, i, v, d, s );
		return nf;
	}
	template <class Quads>
	void aoToHost( Quads quads, int samples, float radius, std::vector<uint32_t>& faceVoxel, std::vector<uint8_t>& faceDir, std::vector<uint16_t>& open, void* stream ) const
	{
		const uint64_t n = quads( 0, nullptr, nullptr, nullptr );
		Out<uint32_t> v( faceVoxel, n, stream );
		Out<uint8_t> d( faceDir, n, stream );
		Out<uint16_t> o( open, n, stream );
		quads( n, v, d, nullptr );
		surfaceAo( n, v, d, samples, radius, o, stream );
		fetch( stream, v, d, o );
	}
	mvrt_svo* m_handle = nullptr;
	bool m_owned = true;
};
} // namespace mvrt
