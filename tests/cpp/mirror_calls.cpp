// mirror_calls.cpp -- the C calls behind the host-vector forms of include/mvrt/IntersectorOctreeGPU.hpp, as text.  A stand-alone host program: it defines the
// mvrt_* entries those forms use itself, as fakes that print one line per call (name, capacities, which device pointers are null and which allocation each of
// the others is, which counters are asked for), hand out numbered allocations and report scripted counts.  It links no library; members it does not call are
// never emitted.  Every form runs once with empty results and once with three entries (the surface forms: 3 faces, 2 rectangles, 5 vertices; components: 7
// voxels, 2 components).  tests/cpp/mirror_calls.txt is what it prints; tests/test_mirror_calls_cpp_cpu.py compares.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "mvrt/IntersectorOctreeGPU.hpp"

namespace
{
uint64_t g_counts[5];	// what the next listing calls report through their counters, in the order of the C signature
uint32_t g_voxels = 0;	// numberOfVoxels of mvrt_svo_get_info
std::map<const void*, std::pair<int, uint64_t>> g_blocks; // address -> (number, bytes), in allocation order
int g_nBlocks = 0;

std::string dev( const void* p ) // a device pointer: "-" = null, "#k:bytes" = allocation k
{
	if( !p ) return "-";
	auto it = g_blocks.find( p );
	if( it == g_blocks.end() ) return "?";
	return "#" + std::to_string( it->second.first ) + ":" + std::to_string( it->second.second );
}
const char* out( const void* p ) { return p ? "out" : "-"; } // a counter
template <class T> void report( T* p, int i )
{
	if( p ) *p = (T)g_counts[i];
}
__attribute__( ( format( printf, 1, 2 ) ) ) void line( const char* fmt, ... )
{
	va_list ap;
	va_start( ap, fmt );
	std::vprintf( fmt, ap );
	va_end( ap );
	std::printf( "\n" );
}
#define D( p ) dev( p ).c_str()
} // namespace

extern "C" {
const char* mvrt_last_error( void ) { return "fake"; }
int mvrt_malloc( void** p, uint64_t bytes )
{
	*p = (void*)( (uintptr_t)0x100000 + 0x1000 * (uintptr_t)g_nBlocks );
	g_blocks[*p] = { g_nBlocks++, bytes };
	line( "  mvrt_malloc %s", D( *p ) );
	return 0;
}
int mvrt_free( void* p )
{
	if( p ) line( "  mvrt_free %s", D( p ) );
	g_blocks.erase( p );
	return 0;
}
int mvrt_memcpy_h2d( void* d, const void* h, uint64_t bytes, void* stream )
{
	line( "  mvrt_memcpy_h2d %s host %s bytes %" PRIu64 " stream %d", D( d ), h ? "given" : "-", bytes, stream != nullptr );
	return 0;
}
int mvrt_memcpy_d2h( void* h, const void* d, uint64_t bytes, void* stream )
{
	line( "  mvrt_memcpy_d2h %s host %s bytes %" PRIu64 " stream %d", D( d ), h ? "given" : "-", bytes, stream != nullptr );
	return 0;
}
int mvrt_svo_create( mvrt_svo** ) { return 1; }
int mvrt_svo_destroy( mvrt_svo* ) { return 1; }
int mvrt_svo_get_info( const mvrt_svo*, mvrt_svo_info* i )
{
	*i = mvrt_svo_info();
	i->numberOfVoxels = g_voxels;
	i->numberOfNodes = 1;
	line( "  mvrt_svo_get_info voxels %u", g_voxels );
	return 0;
}
const void* mvrt_svo_node_buffer_dev( const mvrt_svo* ) { return nullptr; }
const void* mvrt_svo_attribute_buffer_dev( const mvrt_svo* ) { return nullptr; }
int mvrt_svo_build_voxels( mvrt_svo*, const uint32_t* x, const uint32_t* a, uint64_t n, const float*, float dps, int gridRes, int flags, void* )
{
	line( "  mvrt_svo_build_voxels %s %s n %" PRIu64 " dps %g res %d flags %d", D( x ), D( a ), n, dps, gridRes, flags );
	return 0;
}
int mvrt_svo_edit_voxels( mvrt_svo*, const uint32_t* x, const uint32_t* a, const uint8_t* o, uint64_t n, void* )
{
	line( "  mvrt_svo_edit_voxels %s %s %s n %" PRIu64, D( x ), D( a ), D( o ), n );
	return 0;
}
int mvrt_svo_read_voxels( const mvrt_svo*, uint32_t* x, uint32_t* a, void* )
{
	line( "  mvrt_svo_read_voxels %s %s", D( x ), D( a ) );
	return 0;
}
int mvrt_svo_walk_voxels( const mvrt_svo*, uint64_t cap, uint32_t* x, uint32_t* v, uint32_t* a, uint64_t* n, void* )
{
	line( "  mvrt_svo_walk_voxels cap %" PRIu64 " %s %s %s n %s", cap, D( x ), D( v ), D( a ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_enclosed_cells( const mvrt_svo*, uint64_t cap, uint32_t* x, uint32_t* r, uint64_t* n, uint64_t* nr, void* )
{
	line( "  mvrt_svo_enclosed_cells cap %" PRIu64 " %s %s n %s regions %s", cap, D( x ), D( r ), out( n ), out( nr ) );
	report( n, 0 ), report( nr, 1 );
	return 0;
}
int mvrt_svo_enclosed_nearest( const mvrt_svo*, uint64_t cap, uint32_t* x, uint32_t* r, uint32_t* d, uint32_t* v, uint32_t* a, uint64_t* n, uint64_t* nr, void* )
{
	line( "  mvrt_svo_enclosed_nearest cap %" PRIu64 " %s %s %s %s %s n %s regions %s", cap, D( x ), D( r ), D( d ), D( v ), D( a ), out( n ), out( nr ) );
	report( n, 0 ), report( nr, 1 );
	return 0;
}
int mvrt_svo_coarse_voxels( const mvrt_svo*, int down, uint64_t minCount, uint64_t cap, uint32_t* x, uint32_t* a, uint32_t* c, uint64_t* n, void* )
{
	line( "  mvrt_svo_coarse_voxels down %d min %" PRIu64 " cap %" PRIu64 " %s %s %s n %s", down, minCount, cap, D( x ), D( a ), D( c ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_dilation_cells( const mvrt_svo*, int element, uint64_t cap, uint32_t* x, uint32_t* a, uint32_t* c, uint64_t* n, void* )
{
	line( "  mvrt_svo_dilation_cells element %d cap %" PRIu64 " %s %s %s n %s", element, cap, D( x ), D( a ), D( c ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_erosion_voxels( const mvrt_svo*, int element, uint64_t cap, uint32_t* v, uint64_t* n, void* )
{
	line( "  mvrt_svo_erosion_voxels element %d cap %" PRIu64 " %s n %s", element, cap, D( v ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_distance_cells( const mvrt_svo*, uint32_t r2, uint64_t cap, uint32_t* x, uint32_t* d, uint32_t* v, uint32_t* a, uint64_t* n, void* )
{
	line( "  mvrt_svo_distance_cells r2 %u cap %" PRIu64 " %s %s %s %s n %s", r2, cap, D( x ), D( d ), D( v ), D( a ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_depth_voxels( const mvrt_svo*, uint32_t r2, uint64_t cap, uint32_t* v, uint32_t* d, uint64_t* n, void* )
{
	line( "  mvrt_svo_depth_voxels r2 %u cap %" PRIu64 " %s %s n %s", r2, cap, D( v ), D( d ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_components( const mvrt_svo*, int element, uint32_t* l, uint64_t cap, uint32_t* s, uint32_t* f, uint32_t* b, uint64_t* n, uint64_t* big, void* )
{
	line( "  mvrt_svo_components element %d %s cap %" PRIu64 " %s %s %s n %s largest %s", element, D( l ), cap, D( s ), D( f ), D( b ), out( n ), out( big ) );
	report( n, 0 ), report( big, 1 );
	return 0;
}
int mvrt_svo_combine_voxels( const mvrt_svo*, const mvrt_svo* b, int op, const int32_t* offset, uint32_t flags, uint64_t cap, uint32_t* x, uint32_t* a, uint8_t* s, uint64_t* n,
							 uint64_t* overlap, uint64_t* clipped, void* )
{
	line( "  mvrt_svo_combine_voxels b %d op %d offset %s flags %u cap %" PRIu64 " %s %s %s n %s overlap %s clipped %s", b != nullptr, op, offset ? "given" : "-", flags, cap, D( x ),
		  D( a ), D( s ), out( n ), out( overlap ), out( clipped ) );
	report( n, 0 ), report( overlap, 1 ), report( clipped, 2 );
	return 0;
}
int mvrt_svo_nearest_voxels( const mvrt_svo*, uint64_t n, const int32_t* q, uint64_t maxDist2, uint64_t* d, uint32_t* v, uint32_t* a, void* )
{
	line( "  mvrt_svo_nearest_voxels n %" PRIu64 " %s max %" PRIu64 " %s %s %s", n, D( q ), maxDist2, D( d ), D( v ), D( a ) );
	return 0;
}
int mvrt_svo_nearest_between( const mvrt_svo*, const mvrt_svo* b, const int32_t* offset, uint64_t maxDist2, uint64_t cap, uint64_t* d, uint32_t* v, uint64_t* n, uint64_t* md,
							  uint32_t* farthest, uint64_t* nZero, uint64_t* nBeyond, void* )
{
	line( "  mvrt_svo_nearest_between b %d offset %s max %" PRIu64 " cap %" PRIu64 " %s %s n %s maxDist2 %s farthest %s zero %s beyond %s", b != nullptr, offset ? "given" : "-", maxDist2,
		  cap, D( d ), D( v ), out( n ), out( md ), out( farthest ), out( nZero ), out( nBeyond ) );
	report( n, 0 ), report( md, 1 ), report( farthest, 2 ), report( nZero, 3 ), report( nBeyond, 4 );
	return 0;
}
int mvrt_svo_resample_voxels( const mvrt_svo*, const mvrt_cell_transform* xf, int res, uint64_t cap, uint32_t* x, uint32_t* a, uint32_t* s, uint64_t* n, void* )
{
	line( "  mvrt_svo_resample_voxels xf %d res %d cap %" PRIu64 " %s %s %s n %s", xf != nullptr, res, cap, D( x ), D( a ), D( s ), out( n ) );
	report( n, 0 );
	return 0;
}
int mvrt_svo_surface_masks( const mvrt_svo*, uint8_t* m, uint64_t* nf, void* )
{
	line( "  mvrt_svo_surface_masks %s faces %s", D( m ), out( nf ) );
	report( nf, 0 );
	return 0;
}
int mvrt_svo_surface_exterior_masks( const mvrt_svo*, uint8_t* m, uint64_t* nf, uint64_t* nh, void* )
{
	line( "  mvrt_svo_surface_exterior_masks %s faces %s hidden %s", D( m ), out( nf ), out( nh ) );
	report( nf, 0 ), report( nh, 1 );
	return 0;
}
int mvrt_svo_surface_quads( const mvrt_svo*, uint64_t cap, uint32_t* v, uint8_t* d, float* p, uint64_t* nf, void* )
{
	line( "  mvrt_svo_surface_quads cap %" PRIu64 " %s %s %s faces %s", cap, D( v ), D( d ), D( p ), out( nf ) );
	report( nf, 0 );
	return 0;
}
int mvrt_svo_surface_quads_masked( const mvrt_svo*, const uint8_t* m, uint64_t cap, uint32_t* v, uint8_t* d, float* p, uint64_t* nf, void* )
{
	line( "  mvrt_svo_surface_quads_masked %s cap %" PRIu64 " %s %s %s faces %s", D( m ), cap, D( v ), D( d ), D( p ), out( nf ) );
	report( nf, 0 );
	return 0;
}
int mvrt_svo_surface_mesh( const mvrt_svo*, uint64_t fcap, uint64_t vcap, uint32_t* v, uint8_t* d, uint32_t* i, float* x, uint64_t* nf, uint64_t* nv, void* )
{
	line( "  mvrt_svo_surface_mesh cap %" PRIu64 " %" PRIu64 " %s %s %s %s faces %s vertices %s", fcap, vcap, D( v ), D( d ), D( i ), D( x ), out( nf ), out( nv ) );
	report( nf, 0 ), report( nv, 2 );
	return 0;
}
int mvrt_svo_surface_mesh_masked( const mvrt_svo*, const uint8_t* m, uint64_t fcap, uint64_t vcap, uint32_t* v, uint8_t* d, uint32_t* i, float* x, uint64_t* nf, uint64_t* nv, void* )
{
	line( "  mvrt_svo_surface_mesh_masked %s cap %" PRIu64 " %" PRIu64 " %s %s %s %s faces %s vertices %s", D( m ), fcap, vcap, D( v ), D( d ), D( i ), D( x ), out( nf ), out( nv ) );
	report( nf, 0 ), report( nv, 2 );
	return 0;
}
int mvrt_svo_surface_merged( const mvrt_svo*, uint32_t flags, uint64_t rcap, uint64_t vcap, uint32_t* v, uint8_t* d, uint32_t* s, float* p, uint32_t* i, float* x, uint64_t* nf,
							 uint64_t* nr, uint64_t* nv, void* )
{
	line( "  mvrt_svo_surface_merged flags %u cap %" PRIu64 " %" PRIu64 " %s %s %s %s %s %s faces %s rects %s vertices %s", flags, rcap, vcap, D( v ), D( d ), D( s ), D( p ), D( i ),
		  D( x ), out( nf ), out( nr ), out( nv ) );
	report( nf, 0 ), report( nr, 1 ), report( nv, 2 );
	return 0;
}
int mvrt_svo_surface_merged_masked( const mvrt_svo*, const uint8_t* m, uint32_t flags, uint64_t rcap, uint64_t vcap, uint32_t* v, uint8_t* d, uint32_t* s, float* p, uint32_t* i,
									float* x, uint64_t* nf, uint64_t* nr, uint64_t* nv, void* )
{
	line( "  mvrt_svo_surface_merged_masked %s flags %u cap %" PRIu64 " %" PRIu64 " %s %s %s %s %s %s faces %s rects %s vertices %s", D( m ), flags, rcap, vcap, D( v ), D( d ), D( s ),
		  D( p ), D( i ), D( x ), out( nf ), out( nr ), out( nv ) );
	report( nf, 0 ), report( nr, 1 ), report( nv, 2 );
	return 0;
}
int mvrt_svo_surface_ao( const mvrt_svo*, uint64_t n, const uint32_t* v, const uint8_t* d, int samples, float radius, uint16_t* o, void* )
{
	line( "  mvrt_svo_surface_ao faces %" PRIu64 " %s %s samples %d radius %g %s", n, D( v ), D( d ), samples, radius, D( o ) );
	return 0;
}
}

namespace
{
using U32 = std::vector<uint32_t>;
using U8 = std::vector<uint8_t>;
void begin( const char* what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0, uint64_t e = 0 )
{
	const uint64_t v[5] = { a, b, c, d, e };
	for( int i = 0; i < 5; i++ )
		g_counts[i] = v[i];
	g_blocks.clear();
	g_nBlocks = 0;
	std::printf( "%s\n", what );
}
void sizes( std::initializer_list<size_t> s ) // the host vectors afterwards
{
	std::printf( "  sizes" );
	for( size_t v : s )
		std::printf( " %zu", v );
	std::printf( "\n" );
}
} // namespace

int main()
{
	mvrt::IntersectorOctreeGPU o( (mvrt_svo*)0x10 ), b( (mvrt_svo*)0x20 );
	void* const stream = (void*)0x30;
	const int32_t offset[3] = { 1, 2, 3 };
	mvrt_cell_transform xf = mvrt_cell_transform();
	for( uint64_t n : { 0, 3 } )
	{
		std::printf( "==== n = %d\n", (int)n );
		U32 xyz, attribs, vIndex, region, dist2, nearest, count, depth2, source, label, size, first, box;
		U8 source8;
		std::vector<uint64_t> dist64;

		g_voxels = (uint32_t)n;
		begin( "buildFromVoxels" );
		o.buildFromVoxels( U32( n * 3, 1 ), U32( n * 2, 2 ), mvrt::vec3{ 0, 0, 0 }, 0.5f, 8, 1, stream );
		begin( "buildFromVoxels, no attribs" );
		o.buildFromVoxels( U32( n * 3, 1 ), U32(), mvrt::vec3{ 0, 0, 0 }, 0.5f, 8, 0, stream );
		begin( "editVoxels" );
		o.editVoxels( U32( n * 3, 1 ), U32( n * 2, 2 ), U8( n, 1 ), stream );
		begin( "readVoxels" );
		o.readVoxels( xyz, attribs, stream );
		sizes( { xyz.size(), attribs.size() } );
		begin( "surfaceMasks", 9 );
		o.refresh();
		std::printf( "  -> %d\n", (int)o.surfaceMasks( source8, stream ) );
		sizes( { source8.size() } );
		begin( "surfaceExteriorMasks", 9, 2 );
		{
			uint64_t hidden = 0;
			std::printf( "  -> %d", (int)o.surfaceExteriorMasks( source8, &hidden, stream ) );
			std::printf( " hidden %d\n", (int)hidden );
		}
		sizes( { source8.size() } );
		begin( "nearestBetween", n, 40, 6, 1, 2 );
		{
			const auto r = o.nearestBetween( b, offset, 50, dist64, nearest, stream );
			std::printf( "  -> n %d maxDist2 %d farthest %u zero %d beyond %d\n", (int)r.n, (int)r.maxDist2, r.farthest, (int)r.nZero, (int)r.nBeyond );
		}
		sizes( { dist64.size(), nearest.size() } );

		g_voxels = 7;
		o.refresh();
		begin( "walkVoxels", n );
		o.walkVoxels( xyz, vIndex, attribs, stream );
		sizes( { xyz.size(), vIndex.size(), attribs.size() } );
		begin( "enclosedCells", n, 5 );
		std::printf( "  -> %d\n", (int)o.enclosedCells( xyz, region, stream ) );
		sizes( { xyz.size(), region.size() } );
		begin( "enclosedNearest", n, 5 );
		std::printf( "  -> %d\n", (int)o.enclosedNearest( xyz, region, dist2, nearest, attribs, stream ) );
		sizes( { xyz.size(), region.size(), dist2.size(), nearest.size(), attribs.size() } );
		begin( "coarseVoxels", n );
		o.coarseVoxels( 2, 4, xyz, attribs, count, stream );
		sizes( { xyz.size(), attribs.size(), count.size() } );
		begin( "dilationCells", n );
		o.dilationCells( MVRT_MORPH_FACES, xyz, attribs, count, stream );
		sizes( { xyz.size(), attribs.size(), count.size() } );
		begin( "erosionVoxels", n );
		o.erosionVoxels( MVRT_MORPH_CUBE, vIndex, stream );
		sizes( { vIndex.size() } );
		begin( "distanceCells", n );
		o.distanceCells( 9, xyz, dist2, nearest, attribs, stream );
		sizes( { xyz.size(), dist2.size(), nearest.size(), attribs.size() } );
		begin( "depthVoxels", n );
		o.depthVoxels( 9, vIndex, depth2, stream );
		sizes( { vIndex.size(), depth2.size() } );
		begin( "components", n ? 2 : 0, 4 );
		o.components( MVRT_MORPH_FACES, label, size, first, box, stream );
		sizes( { label.size(), size.size(), first.size(), box.size() } );
		begin( "combineVoxels", n, 11, 12 );
		{
			uint64_t overlap = 0, clipped = 0;
			o.combineVoxels( b, MVRT_COMBINE_XOR, offset, MVRT_COMBINE_ATTRIB_B, xyz, attribs, source8, &overlap, &clipped, stream );
			std::printf( "  -> overlap %d clipped %d\n", (int)overlap, (int)clipped );
		}
		sizes( { xyz.size(), attribs.size(), source8.size() } );
		begin( "combineVoxels, no counters" );
		g_counts[0] = n;
		o.combineVoxels( b, MVRT_COMBINE_UNION, nullptr, 0, xyz, attribs, source8, nullptr, nullptr, stream );
		begin( "nearestVoxels" );
		o.nearestVoxels( std::vector<int32_t>( n * 3, 1 ), 50, dist64, nearest, attribs, stream );
		sizes( { dist64.size(), nearest.size(), attribs.size() } );
		begin( "resampleVoxels", n );
		o.resampleVoxels( xf, 8, xyz, attribs, source, stream );
		sizes( { xyz.size(), attribs.size(), source.size() } );

		// the surface forms: faces, rectangles, vertices
		const uint64_t nf = n ? 3 : 0, nr = n ? 2 : 0, nv = n ? 5 : 0;
		const U8 masks( 7, 0x3f );
		U32 faceVoxel, indices, rectSize;
		U8 faceDir;
		std::vector<float> positions, vertices;
		std::vector<uint16_t> open;
		begin( "surfaceQuads", nf );
		o.surfaceQuads( faceVoxel, faceDir, positions, stream );
		sizes( { faceVoxel.size(), faceDir.size(), positions.size() } );
		begin( "surfaceQuadsMasked", nf );
		o.surfaceQuadsMasked( masks, faceVoxel, faceDir, positions, stream );
		sizes( { faceVoxel.size(), faceDir.size(), positions.size() } );
		begin( "surfaceMesh", nf, 0, nv );
		o.surfaceMesh( vertices, indices, faceVoxel, faceDir, stream );
		sizes( { vertices.size(), indices.size(), faceVoxel.size(), faceDir.size() } );
		begin( "surfaceMeshMasked", nf, 0, nv );
		o.surfaceMeshMasked( masks, vertices, indices, faceVoxel, faceDir, stream );
		sizes( { vertices.size(), indices.size(), faceVoxel.size(), faceDir.size() } );
		for( uint32_t flags : { (uint32_t)MVRT_SURFACE_MERGE_ANY_ATTRIBUTE, (uint32_t)( MVRT_SURFACE_MERGE_ANY_ATTRIBUTE | MVRT_SURFACE_MERGE_WELD ) } )
		{
			begin( "surfaceMerged", nf, nr, nv );
			std::printf( "  -> %d\n", (int)o.surfaceMerged( flags, vertices, indices, faceVoxel, faceDir, rectSize, stream ) );
			sizes( { vertices.size(), indices.size(), faceVoxel.size(), faceDir.size(), rectSize.size() } );
			begin( "surfaceMergedMasked", nf, nr, nv );
			std::printf( "  -> %d\n", (int)o.surfaceMergedMasked( masks, flags, vertices, indices, faceVoxel, faceDir, rectSize, stream ) );
			sizes( { vertices.size(), indices.size(), faceVoxel.size(), faceDir.size(), rectSize.size() } );
		}
		begin( "surfaceAo", nf );
		o.surfaceAo( 4, 0.5f, faceVoxel, faceDir, open, stream );
		sizes( { faceVoxel.size(), faceDir.size(), open.size() } );
		begin( "surfaceAoMasked", nf );
		o.surfaceAoMasked( masks, 4, 0.5f, faceVoxel, faceDir, open, stream );
		sizes( { faceVoxel.size(), faceDir.size(), open.size() } );
	}
	return 0;
}
