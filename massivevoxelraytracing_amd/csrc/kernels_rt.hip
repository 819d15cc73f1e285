// kernels_rt.hip -- the hot path: octree traversal, primary cast, wavefront path tracer with stable
// live-path compaction.  Hand-written for gfx950 (wave64, LDS stacks, SoA buffers).
//
// Reference semantics (what each kernel must reproduce): /root/reference/voxKernel.cu:437-483 (render),
// :610-777 (renderPT), voxCommon.hpp:231-423 (traversal), StreamCompaction.hpp:87-184 (stable compaction).
#include <stdlib.h>

#include <type_traits>

#include "launch.h"
#include "traverse_stream.h"

#define WAVE 64
#define CBLOCK 256 // paths per compaction block

MVRT_DI uint32_t laneId() { return __builtin_amdgcn_mbcnt_hi( ~0u, __builtin_amdgcn_mbcnt_lo( ~0u, 0u ) ); }

MVRT_DI unsigned long long waveSum( unsigned long long v )
{
	for( int o = 32; o > 0; o >>= 1 ) v += __shfl_down( v, o, WAVE );
	return v;
}

static int numCUs();

// =====================================================================================================
// Persistent-wave ("stream") variants for embedded-mask octrees: traverse_stream.h
// =====================================================================================================
#define STREAM_WAVES_PER_CU 32

struct BatchIO
{
	const float *rox, *roy, *roz, *rdx, *rdy, *rdz;
	const uint8_t* isShadow;
	float* tOut;
	int32_t* nMajorOut;
	uint64_t* pathOut; // scratch: resolved to vIndex by kResolveVIndex
	uint32_t* descentsOut;
	MVRT_UTIL_COUNTERS
	const uint64_t* originPath; // optional: per ray, the full path of an existing voxel (start-below-the-root hint), ~0 = none
	uint32_t levels;
	MVRT_DI bool load( uint32_t i, f3* ro, f3* rd, uint32_t* hint ) const
	{
		*ro = mk3( rox[i], roy[i], roz[i] );
		*rd = mk3( rdx[i], rdy[i], rdz[i] );
		if( originPath )
		{
			const uint64_t op = originPath[i];
			if( op != ~0ull ) *hint = hintFromVoxelPath( op, levels );
		}
		return isShadow ? isShadow[i] != 0 : false;
	}
	MVRT_DI void store( uint32_t i, const StreamHit& h, bool ) const
	{
		tOut[i] = h.t;
		if( nMajorOut ) nMajorOut[i] = h.nMajor;
		if( pathOut ) pathOut[i] = h.path;
		if( descentsOut ) descentsOut[i] = h.descents;
	}
};
// dense post-pass: vIndex (and optionally the primary-cast colour) from the recorded voxel paths
__global__ void __launch_bounds__( 256 ) kResolveVIndex( SvoDev svo, uint64_t n, const float* __restrict__ t, const uint64_t* __restrict__ path, const uint8_t* __restrict__ isShadow,
														  uint32_t* __restrict__ vIndexOut, uchar4* __restrict__ colorOut )
{
	for( uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256 )
	{
		uint32_t v = 0;
		const bool hit = t[i] != MVRT_MAXF;
		if( hit && !( isShadow && isShadow[i] ) ) v = voxelIndexFromPath( svo, path[i] );
		if( vIndexOut ) vIndexOut[i] = v;
		if( colorOut && hit )
		{
			uint32_t col = svo.attrs[v].x; // IntersectorOctreeGPU::getVoxelColor, voxKernel.cu:466
			colorOut[i] = make_uchar4( col & 0xFF, ( col >> 8 ) & 0xFF, ( col >> 16 ) & 0xFF, ( col >> 24 ) & 0xFF );
		}
	}
}
#ifndef MVRT_TRACE_WAVES
#define MVRT_TRACE_WAVES 7 // waves per SIMD the traversal kernels are register-budgeted for (72 VGPRs)
#endif
// the embedded flavour's 8 KiB LDS ring admits 5 waves per SIMD (5, 6 and 7 perform alike on cache-resident octrees, profiles/r02_traversal_experiments.txt)
#ifndef MVRT_TREE_WAVES
#define MVRT_TREE_WAVES ( MVRT_RING_TREE >= 8 ? 3 : 6 )
#endif
// ... and the tree flavour's 12 KiB per wave (8-slot ring + two mask words per slot) 3
#define MVRT_WAVES_OF( FL ) ( ( FL ) == 0 && MVRT_RING_EMBED >= 8 && MVRT_TRACE_WAVES > 40 / MVRT_RING_EMBED ? 40 / MVRT_RING_EMBED : ( ( FL ) == 2 && MVRT_TRACE_WAVES > MVRT_TREE_WAVES ? MVRT_TREE_WAVES : MVRT_TRACE_WAVES ) )
template <int FL>
__global__ void __launch_bounds__( 64, MVRT_WAVES_OF( FL ) ) kTraceBatchStream( SvoDev svo, uint64_t n, BatchIO io, TraceWorkspace ws, uint32_t chunk )
{
	traceStream<FL>( makeTraceCore( svo ), io, n, ws.cursor, chunk, ws );
}

struct PrimaryIO
{
	SvoDev svo;
	CameraPinhole cam;
	int W, H, showVertexColor;
	uchar4* rgba;
	float* tOut;
	int32_t* nMajorOut;
	uint64_t* pathOut;
	uint32_t* descentsOut;
	MVRT_UTIL_COUNTERS
	f3 rdKeep; // direction of the ray this lane is tracing (for the normal colour)
	MVRT_DI bool load( uint32_t pixelIdx, f3* ro, f3* rd, uint32_t* )
	{
		int x = (int)( pixelIdx % W );
		int y = (int)( pixelIdx / W );
		cameraShoot( cam, ro, rd, x, y, 0.5f, 0.5f, W, H ); // voxKernel.cu:455
		rdKeep = *rd;
		return false;
	}
	MVRT_DI void store( uint32_t pixelIdx, const StreamHit& r, bool ) const
	{
		uchar4 c = make_uchar4( 0, 0, 0, 255 );
		if( r.t != MVRT_MAXF ) // voxKernel.cu:462-478
		{
			if( !showVertexColor ) // the vertex-colour case is filled in by kResolveVIndex
			{
				f3 hn = getHitN( r.nMajor, rdKeep );
				f3 color = ( hn + mk3( 1.0f, 1.0f, 1.0f ) ) * 0.5f;
				c = make_uchar4( (uint8_t)( 255 * color.x + 0.5f ), (uint8_t)( 255 * color.y + 0.5f ), (uint8_t)( 255 * color.z + 0.5f ), 255 );
			}
		}
		if( rgba ) rgba[pixelIdx] = c;
		if( tOut ) tOut[pixelIdx] = r.t;
		if( nMajorOut ) nMajorOut[pixelIdx] = r.nMajor;
		if( pathOut ) pathOut[pixelIdx] = r.path;
		if( descentsOut ) descentsOut[pixelIdx] = r.descents;
	}
};
template <int FL>
__global__ void __launch_bounds__( 64, MVRT_WAVES_OF( FL ) ) kRenderPrimaryStream( PrimaryIO io, TraceWorkspace ws, uint32_t chunk )
{
	traceStream<FL>( makeTraceCore( io.svo ), io, (uint64_t)io.W * io.H, ws.cursor, chunk, ws );
}

static uint32_t streamChunk( uint64_t total, uint64_t waves )
{
	uint64_t c = total / ( waves * 4 );
	c = ( c + 63 ) / 64 * 64;
#ifndef MVRT_CHUNK_MAX
#define MVRT_CHUNK_MAX 512 // rays per grab (1024 / 512 / 256: a launch alone 5885 / 6127 / 6152 Mrays/s -- finer grabs balance its end; pipelined job unchanged)
#endif
	if( c < 64 ) c = 64;
	if( c > MVRT_CHUNK_MAX ) c = MVRT_CHUNK_MAX;
	return (uint32_t)c;
}
static int streamGrid( uint64_t total, int nCUs )
{
	uint64_t need = ( total + 63 ) / 64;
	uint64_t cap = (uint64_t)nCUs * STREAM_WAVES_PER_CU;
	if( need < 1 ) need = 1;
	return (int)( need < cap ? need : cap );
}
// launches whose ray count the host knows (batch API, primary cast): the small-launch rule of the path tracer (kPtTraceStream) applied to the
// grid itself -- total / (64 * 8) waves, at least two per SIMD (primary cast 1920x1080 at 1024^3: 0.644 -> 0.46 ms)
static int streamGridKnown( uint64_t total, int nCUs )
{
	const uint64_t full = (uint64_t)streamGrid( total, nCUs );
#ifndef MVRT_KNOWN_RPL
#define MVRT_KNOWN_RPL 8
#endif
#ifndef MVRT_KNOWN_MINPCU
#define MVRT_KNOWN_MINPCU 8
#endif
	uint64_t want = total / ( 64ull * MVRT_KNOWN_RPL ) + 1;
	if( want < (uint64_t)nCUs * MVRT_KNOWN_MINPCU ) want = (uint64_t)nCUs * MVRT_KNOWN_MINPCU;
	return (int)( want < full ? want : full );
}
// lane capacity of a traversal workspace = row stride of the spill rows; rounded up to a power of two so that the kernel
// addresses row L of a lane with one shift-add on a 32-bit offset (traverse_stream.h)
uint64_t traceWorkspaceLanes()
{
	uint64_t lanes = (uint64_t)numCUs() * STREAM_WAVES_PER_CU * 64, p = 64;
	while( p < lanes ) p <<= 1;
	return p;
}

// =====================================================================================================
// mvrt_trace_batch: host-callable batch form of IntersectorOctreeGPU::intersect
// =====================================================================================================
static int persistentGrid( uint64_t items, int block, int numCUs, int blocksPerCU )
{
	uint64_t need = ( items + block - 1 ) / block;
	uint64_t cap = (uint64_t)numCUs * blocksPerCU;
	if( need < 1 ) need = 1;
	return (int)( need < cap ? need : cap );
}

static int g_numCUs = 0;
static int numCUs()
{
	if( g_numCUs == 0 )
	{
		int dev = 0;
		hipDeviceProp_t p;
		if( hipGetDevice( &dev ) == hipSuccess && hipGetDeviceProperties( &p, dev ) == hipSuccess ) g_numCUs = p.multiProcessorCount;
		if( g_numCUs <= 0 ) g_numCUs = 256;
	}
	return g_numCUs;
}

// the traversal flavour of an octree (traverse_stream.h) as a compile-time constant: calls f( std::integral_constant<int, FL>() )
template <class F>
static void withFlavour( const SvoDev& svo, F&& f )
{
	if( svo.embedded ) f( std::integral_constant<int, 0>() );
	else if( svo.tree ) f( std::integral_constant<int, 2>() );
	else f( std::integral_constant<int, 1>() );
}

int launchTraceBatch( const SvoDev& svo, const TraceWorkspace& ws, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy,
					  const float* rdz, const uint8_t* isShadow, float* t, int32_t* nMajor, uint32_t* vIndex, uint32_t* descents, hipStream_t stream, const uint64_t* originPath )
{
	if( n == 0 ) return 0;
	if( ws.spill )
	{
		uint64_t* paths = vIndex ? ws.paths : nullptr;
		if( vIndex && ws.pathCap < n )
		{
			mvrtSetError( "internal: path scratch too small" );
			return 1;
		}
		BatchIO io = { rox, roy, roz, rdx, rdy, rdz, isShadow, t, nMajor, paths, descents };
		io.originPath = svo.embedded ? originPath : nullptr;
		io.levels = svo.levels;
		int grid = streamGridKnown( n, numCUs() );
		MVRT_HIP( hipMemsetAsync( ws.cursor, 0, 8, stream ) );
		withFlavour( svo, [&]( auto fl ) { hipLaunchKernelGGL( kTraceBatchStream<decltype( fl )::value>, dim3( grid ), dim3( 64 ), 0, stream, svo, n, io, ws, streamChunk( n, grid ) ); } );
		if( vIndex )
			hipLaunchKernelGGL( kResolveVIndex, dim3( persistentGrid( n, 256, numCUs(), 8 ) ), dim3( 256 ), 0, stream, svo, n, t, paths, isShadow, vIndex, (uchar4*)nullptr );
		MVRT_HIP( hipGetLastError() );
		return 0;
	}
	mvrtSetError( "internal: traversal workspace missing" );
	return 1;
}

// =====================================================================================================
// mvrt_render_primary: the `render` kernel (voxKernel.cu:437-483)
// =====================================================================================================
int launchRenderPrimary( const SvoDev& svo, const TraceWorkspace& ws, const CameraPinhole& cam, int W, int H, int showVertexColor, uchar4* rgba, float* t,
						 int32_t* nMajor, uint32_t* vIndex, uint32_t* descents, hipStream_t stream )
{
	uint64_t n = (uint64_t)W * H;
	if( n == 0 ) return 0;
	if( ws.spill )
	{
		PrimaryIO io;
		io.svo = svo;
		io.cam = cam;
		io.W = W;
		io.H = H;
		io.showVertexColor = showVertexColor;
		io.rgba = rgba;
		io.tOut = t;
		io.nMajorOut = nMajor;
		const bool needPaths = vIndex || ( showVertexColor && rgba );
		if( needPaths && ( ws.pathCap < n || !t ) )
		{
			mvrtSetError( "internal: path scratch too small" );
			return 1;
		}
		io.pathOut = needPaths ? ws.paths : nullptr;
		io.descentsOut = descents;
		io.rdKeep = mk3( 0, 0, 0 );
		int grid = streamGridKnown( n, numCUs() );
		MVRT_HIP( hipMemsetAsync( ws.cursor, 0, 8, stream ) );
		withFlavour( svo, [&]( auto fl ) { hipLaunchKernelGGL( kRenderPrimaryStream<decltype( fl )::value>, dim3( grid ), dim3( 64 ), 0, stream, io, ws, streamChunk( n, grid ) ); } );
		if( needPaths )
			hipLaunchKernelGGL( kResolveVIndex, dim3( persistentGrid( n, 256, numCUs(), 8 ) ), dim3( 256 ), 0, stream, svo, n, t, ws.paths, (const uint8_t*)nullptr, vIndex,
								showVertexColor ? rgba : (uchar4*)nullptr );
		MVRT_HIP( hipGetLastError() );
		return 0;
	}
	mvrtSetError( "internal: traversal workspace missing" );
	return 1;
}

// =====================================================================================================
// Stable compaction: count per 256-item virtual block -> single-workgroup exclusive scan -> rank
// =====================================================================================================
// number of set flags in each 256-item block
template <class Pred>
MVRT_DI void blockCountBody( Pred pred, uint64_t n, uint32_t* __restrict__ blockCount )
{
	__shared__ uint32_t waveCnt[CBLOCK / WAVE];
	const uint64_t nBlocks = ( n + CBLOCK - 1 ) / CBLOCK;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * CBLOCK + threadIdx.x;
		bool keep = i < n ? pred( i ) : false;
		unsigned long long b = __ballot( keep );
		if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) waveCnt[threadIdx.x / WAVE] = __popcll( b );
		__syncthreads();
		if( threadIdx.x == 0 ) blockCount[vb] = waveCnt[0] + waveCnt[1] + waveCnt[2] + waveCnt[3];
		__syncthreads();
	}
}

// in-block stable rank of a kept item; every thread of the block must call it
MVRT_DI uint32_t blockRank( bool keep, uint32_t* waveCnt /* LDS, 4 entries */ )
{
	unsigned long long b = __ballot( keep );
	uint32_t lane = threadIdx.x & ( WAVE - 1 );
	uint32_t w = threadIdx.x / WAVE;
	uint32_t inWave = __popcll( b & ( ( 1ull << lane ) - 1ull ) );
	if( lane == 0 ) waveCnt[w] = __popcll( b );
	__syncthreads();
	uint32_t off = 0;
	for( uint32_t k = 0; k < w; k++ ) off += waveCnt[k];
	__syncthreads();
	return off + inWave;
}

// The survivor scan: two launches of one-wave workgroups that declare NO LDS and never wait for one another (a launch boundary is the only ordering).
//   kScanTiles: wave t scans tile t -- MVRT_SCAN_TILE (T = 256) consecutive block counts -- in place and writes the tile's sum to tileBase[t];
//   kScanTop:   one wave scans the tile sums in place, 256 (C: 64 lanes x 4) per iteration with a running carry, and writes the grand total.
// The offset of block vb is then blockCount[vb] + tileBase[vb / T] (scanOffset).  Every lane owns four consecutive entries: one 16-byte load and store, coalesced;
// both arrays are padded to whole quads (scanCountEntries / scanTileEntries, launch.h).  The item count is read from device memory when nItemsDev != null:
// the grid is sized for the host's upper bound and tiles past the end exit.
// Why one-wave workgroups without LDS: the persistent traversal waves of the sibling pass hold all 160 KiB of a CU's LDS and all but 112 VGPRs of every SIMD
// until their launch tail; a single wave that asks for no LDS is the unit that still finds a slot there.
#define SCAN_TOP_TILES 256 // C: tile sums one kScanTop iteration takes
// exclusive scan, in place and plus `carry`, of the up to 256 entries a[base .. min( base + 256, n )) by one wave; returns their sum to every lane
MVRT_DI uint32_t waveScan256( uint32_t* __restrict__ a, uint32_t base, uint32_t n, uint32_t lane, uint32_t carry )
{
	const uint32_t i0 = base + lane * 4;
	uint4 c = make_uint4( 0u, 0u, 0u, 0u );
	if( i0 < n ) c = *(const uint4*)( a + i0 ); // entries past n inside the last quad are padding: masked below
	if( i0 + 1 >= n ) c.y = 0u;
	if( i0 + 2 >= n ) c.z = 0u;
	if( i0 + 3 >= n ) c.w = 0u;
	const uint32_t mine = c.x + c.y + c.z + c.w;
	uint32_t incl = mine; // inclusive scan of the lane sums
	for( int o = 1; o < WAVE; o <<= 1 )
	{
		const uint32_t v = __shfl_up( incl, o, WAVE );
		if( (int)lane >= o ) incl += v;
	}
	const uint32_t e0 = carry + incl - mine;
	if( i0 + 3 < n ) *(uint4*)( a + i0 ) = make_uint4( e0, e0 + c.x, e0 + c.x + c.y, e0 + c.x + c.y + c.z );
	else if( i0 < n ) // the last, partial quad: nothing is written past n
	{
		a[i0] = e0;
		if( i0 + 1 < n ) a[i0 + 1] = e0 + c.x;
		if( i0 + 2 < n ) a[i0 + 2] = e0 + c.x + c.y;
	}
	return __shfl( incl, WAVE - 1, WAVE );
}
__global__ void __launch_bounds__( WAVE ) kScanTiles( uint32_t* __restrict__ blockCount, uint64_t nItemsHost, const uint32_t* __restrict__ nItemsDev, uint32_t* __restrict__ tileBase )
{
	const uint64_t nItems = nItemsDev ? (uint64_t)*nItemsDev : nItemsHost;
	const uint32_t nBlocks = (uint32_t)( ( nItems + CBLOCK - 1 ) / CBLOCK );
	const uint32_t nTiles = ( nBlocks + MVRT_SCAN_TILE - 1 ) / MVRT_SCAN_TILE;
	for( uint32_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x )
	{
		const uint32_t sum = waveScan256( blockCount, tile * MVRT_SCAN_TILE, nBlocks, threadIdx.x, 0u );
		if( threadIdx.x == 0 ) tileBase[tile] = sum;
	}
}
__global__ void __launch_bounds__( WAVE ) kScanTop( uint32_t* __restrict__ tileBase, uint64_t nItemsHost, const uint32_t* __restrict__ nItemsDev, uint32_t* __restrict__ totalOut,
													unsigned long long* __restrict__ rayStats, int nKinds, int shadowKind )
{
	const uint64_t nItems = nItemsDev ? (uint64_t)*nItemsDev : nItemsHost;
	if( rayStats && threadIdx.x == 0 ) // ray accounting of the stage that was just traced (intersect() calls)
	{
		atomicAdd( &rayStats[0], (unsigned long long)nItems * nKinds );
		if( shadowKind ) atomicAdd( &rayStats[1], (unsigned long long)nItems );
	}
	const uint32_t nBlocks = (uint32_t)( ( nItems + CBLOCK - 1 ) / CBLOCK );
	const uint32_t nTiles = ( nBlocks + MVRT_SCAN_TILE - 1 ) / MVRT_SCAN_TILE;
	uint32_t carry = 0;
	for( uint32_t base = 0; base < nTiles; base += SCAN_TOP_TILES ) carry += waveScan256( tileBase, base, nTiles, threadIdx.x, carry );
	if( threadIdx.x == 0 && totalOut ) *totalOut = carry;
}
// first stable slot of block vb after the two launches
MVRT_DI uint32_t scanOffset( const uint32_t* __restrict__ blockCount, const uint32_t* __restrict__ tileBase, uint64_t vb ) { return blockCount[vb] + tileBase[vb / MVRT_SCAN_TILE]; }
// nItems: the host's count or, with nItemsDev, its upper bound
static void launchScan( uint32_t* blockCount, uint32_t* tileBase, uint64_t nItems, const uint32_t* nItemsDev, uint32_t* totalOut, unsigned long long* rayStats, int nKinds, int shadowKind,
						hipStream_t stream )
{
	const uint64_t nBlocks = ( nItems + CBLOCK - 1 ) / CBLOCK, nTiles = ( nBlocks + MVRT_SCAN_TILE - 1 ) / MVRT_SCAN_TILE;
	hipLaunchKernelGGL( kScanTiles, dim3( (uint32_t)( nTiles ? nTiles : 1 ) ), dim3( WAVE ), 0, stream, blockCount, nItemsDev ? (uint64_t)0 : nItems, nItemsDev, tileBase );
	hipLaunchKernelGGL( kScanTop, dim3( 1 ), dim3( WAVE ), 0, stream, tileBase, nItemsDev ? (uint64_t)0 : nItems, nItemsDev, totalOut, rayStats, nKinds, shadowKind );
}

__global__ void __launch_bounds__( CBLOCK ) kCountFlags( const uint8_t* __restrict__ keep, uint64_t n, uint32_t* __restrict__ blockCount )
{
	blockCountBody( [=]( uint64_t i ) { return keep[i] != 0; }, n, blockCount );
}
__global__ void __launch_bounds__( CBLOCK ) kRankFlags( const uint8_t* __restrict__ keep, uint64_t n, const uint32_t* __restrict__ blockOffset, const uint32_t* __restrict__ tileBase,
													   uint32_t* __restrict__ dstIndex )
{
	__shared__ uint32_t waveCnt[CBLOCK / WAVE];
	const uint64_t nBlocks = ( n + CBLOCK - 1 ) / CBLOCK;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * CBLOCK + threadIdx.x;
		bool k = i < n ? keep[i] != 0 : false;
		uint32_t r = blockRank( k, waveCnt );
		if( i < n ) dstIndex[i] = k ? scanOffset( blockOffset, tileBase, vb ) + r : 0xFFFFFFFFu;
	}
}

// blockScratch: scanCountEntries( n ) + scanTileEntries( n ) entries, 16-byte aligned
int launchCompactIndices( const uint8_t* keep, uint64_t n, uint32_t* dstIndex, uint32_t* kept, uint32_t* blockScratch, hipStream_t stream )
{
	int grid = persistentGrid( n, CBLOCK, numCUs(), 8 );
	uint32_t* tileBase = blockScratch + scanCountEntries( n );
	hipLaunchKernelGGL( kCountFlags, dim3( grid ), dim3( CBLOCK ), 0, stream, keep, n, blockScratch );
	launchScan( blockScratch, tileBase, n, nullptr, kept, nullptr, 0, 0, stream );
	hipLaunchKernelGGL( kRankFlags, dim3( grid ), dim3( CBLOCK ), 0, stream, keep, n, blockScratch, tileBase, dstIndex );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// =====================================================================================================
// Wavefront path tracer
// =====================================================================================================
struct PtParams
{
	SvoDev svo;
	HdriDev hdri;
	const float2* pmj;
	CameraPinhole cams[MVRT_MAX_BATCH]; // one camera per merged step
	PtFrame frame;
	PtBuffers buf;
	int hdriEnabled;  // hdri.isEnabled(), renderCommon.hpp:467-470
	int extraSamples; // nSampleExtraDirect = hasEmission ? 1 : 0, voxKernel.cu:721
	int useHints;	  // secondary rays start below the root (traverse_stream.h); 0 = every ray from the root (A/B, tests)
};

// owned (local) pixel -> global pixel index.  Blocks of 256 pixels dealt round-robin over tiles.
MVRT_DI uint32_t globalPixel( const PtFrame& f, uint32_t localPixel )
{
	uint32_t lb = localPixel / MVRT_TILE_PIXELS;
	return ( lb * f.tileCount + f.tileIndex ) * MVRT_TILE_PIXELS + ( localPixel % MVRT_TILE_PIXELS );
}

// sample id ("task") of a batch of nSteps merged steps: ((step * validOwnedPixels + localPixel) * 16 + localSpp)
MVRT_DI void decodeTask( const PtFrame& f, uint32_t task, uint32_t* step, uint32_t* localPixel, uint32_t* localSpp )
{
	const uint32_t ps = task / MVRT_SPP_PER_STEP;
	*localSpp = task % MVRT_SPP_PER_STEP;
	const uint32_t vp = (uint32_t)f.validOwnedPixels;
	*step = ps / vp;
	*localPixel = ps - *step * vp;
}

// number of PMJ dimensions consumed before the shading of depth k (voxKernel.cu:662-666,699-700,724,741)
MVRT_DI int dimBase( int k, int hdriEnabled, int extraSamples ) { return 2 + k * ( ( hdriEnabled ? 2 : 0 ) + 1 ) + ( k > 0 ? extraSamples : 0 ); }

// Sample mask (mvrt_pt_set_sample_mask): a pass restricted to the active pixels numbers its tasks over the ACTIVE LIST -- PtFrame::validOwnedPixels is the
// number of active pixels and decodeTask's pixel is a slot of the list -- and the kernels that turn a task into a pixel look the owned pixel up here.  They
// are instantiated twice; the unmasked instantiation keeps the kernel's arguments and compiles to the instructions it had without the mask.
// The kernels take the list as a trailing parameter PACK (`ACTIVE... active`): empty for the unmasked instantiation, one `const uint32_t*` for the masked one.
MVRT_DI uint32_t slotPixel( uint32_t slot ) { return slot; }
MVRT_DI uint32_t slotPixel( uint32_t slot, const uint32_t* active ) { return active[slot]; }

// ---- generate: camera samples -> primary rays (voxKernel.cu:635-667) -------------------------------
template <class... ACTIVE>
__global__ void __launch_bounds__( 256 ) kPtGenerate( PtParams P, ACTIVE... active )
{
	const uint64_t n = P.frame.validOwnedPixels * MVRT_SPP_PER_STEP * P.frame.nSteps;
	const PathSet& o = P.buf.set[0];
	for( uint64_t task = (uint64_t)blockIdx.x * 256 + threadIdx.x; task < n; task += (uint64_t)gridDim.x * 256 )
	{
		uint32_t step, localPixel, localSpp;
		decodeTask( P.frame, (uint32_t)task, &step, &localPixel, &localSpp );
		uint32_t pixelIdx = globalPixel( P.frame, slotPixel( localPixel, active... ) );
		int x = pixelIdx % P.frame.width;
		int y = pixelIdx / P.frame.width;
		uint32_t spp = ( P.frame.iteration + step ) * MVRT_SPP_PER_STEP + localSpp; // voxKernel.cu:642
		uint32_t stream = hashCombine2( 0u, pixelIdx );
		f2 camU = pmjSample2d( P.pmj, spp, 0, stream );
		f2 lensU = pmjSample2d( P.pmj, spp, 1, stream );
		f3 ro, rd;
		cameraShootThinLens( P.cams[step], &ro, &rd, x, y, camU.x, camU.y, P.frame.width, P.frame.height, lensU.x, lensU.y );
		o.task[task] = (uint32_t)task;
		o.rox[task] = ro.x;
		o.roy[task] = ro.y;
		o.roz[task] = ro.z;
		o.rdx[task] = rd.x;
		o.rdy[task] = rd.y;
		o.rdz[task] = rd.z;
	}
	for( uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < ( n + CBLOCK - 1 ) / CBLOCK; b += (uint64_t)gridDim.x * 256 ) P.buf.blockCount[b] = 0u;
	if( blockIdx.x == 0 && threadIdx.x == 0 )
	{
		P.buf.liveCount[0] = (uint32_t)n;
		for( int k = 0; k < 16; k++ ) P.buf.cursors[k] = 0ull; // per-stage ray cursors of the persistent traversal waves
		atomicAdd( &P.buf.stats[5], (unsigned long long)n );
	}
}

// ---- trace: all rays of one stage.  Ray r = kind * n + path; kind 0 bounce/primary, 1 shadow, 2 extra -
// Opaque view of a kernarg pointer: the asm makes the value unknown to the optimiser at this point, so the ~25 array
// pointers read through it are (re)loaded with scalar loads where they are used -- at refill time -- instead of being
// hoisted out of the traversal loop, where they would occupy ~60 SGPRs and push the node pointer out of registers.
// The table is written by the host before the launch and never by a kernel: it is read through the CONSTANT address space, so the
// pointer fetches are scalar loads that the compiler may batch freely (as plain global loads each of them had to be re-fetched, and
// waited for, after every result store that might alias the table: ~9 dependent memory round trips per refill instead of ~3).
template <class T>
MVRT_DI const __attribute__( ( address_space( 4 ) ) ) T* opaquePtr( const T* p )
{
	asm volatile( "" : "+s"( p ) );
	return (const __attribute__( ( address_space( 4 ) ) ) T*)p;
}

struct PtIO
{
	const PtBuffers* table; // device-resident pointer table (read through opaquePtr)
	int setIdx;
	uint32_t n;
	int shadowKind;
	int useHint; // stage > 0 on an embedded-mask octree: PathSet::org holds the start-below-the-root hint of every path
	MVRT_UTIL_COUNTERS
	uint32_t dNormal, dShadow, nHits; // per-lane tallies (a lane sees far fewer than 2^32 descents per launch)
	MVRT_DI int kindOf( uint32_t r, uint32_t* i ) const
	{
		const uint32_t kindSlot = ( r >= n ? 1u : 0u ) + ( r >= 2u * n ? 1u : 0u );
		*i = r - ( kindSlot == 0u ? 0u : ( kindSlot == 1u ? n : 2u * n ) ); // (no integer multiply: quarter rate)
		return kindSlot == 0 ? 0 : ( kindSlot == 1 ? ( shadowKind ? 1 : 2 ) : 2 );
	}
	MVRT_DI bool load( uint32_t r, f3* ro, f3* rd, uint32_t* hint ) const
	{
		const __attribute__( ( address_space( 4 ) ) ) PtBuffers& buf = *opaquePtr( table );
		const __attribute__( ( address_space( 4 ) ) ) PathSet& in = buf.set[setIdx];
		uint32_t i;
		const int kind = kindOf( r, &i );
		*ro = mk3( in.rox[i], in.roy[i], in.roz[i] );
		if( useHint ) *hint = in.org[i]; // every ray of a path starts on the voxel the path hit last
		// the direction arrays of the three kinds: all nine pointers are fetched (one batch of scalar loads from the table) and the lane picks its three with
		// selects.  As an if / else chain over the kinds every arm fetched its own pointers behind a divergent branch and waited for them there, and the third
		// pointer came through a per-lane vector load that the direction load then had to wait for -- a second memory round trip in every refill
		const float *x0 = in.rdx, *y0 = in.rdy, *z0 = in.rdz, *x1 = buf.sx, *y1 = buf.sy, *z1 = buf.sz, *x2 = buf.ex, *y2 = buf.ey, *z2 = buf.ez;
		const float* const px = kind == 0 ? x0 : ( kind == 1 ? x1 : x2 );
		const float* const py = kind == 0 ? y0 : ( kind == 1 ? y1 : y2 );
		const float* const pz = kind == 0 ? z0 : ( kind == 1 ? z1 : z2 );
		*rd = mk3( px[i], py[i], pz[i] );
		return kind == 1;
	}
	MVRT_DI void store( uint32_t r, const StreamHit& h, bool )
	{
		const __attribute__( ( address_space( 4 ) ) ) PtBuffers& buf = *opaquePtr( table );
		uint32_t i;
		const int kind = kindOf( r, &i );
		const bool isHit = h.t != MVRT_MAXF;
		if( kind == 0 )
		{
			buf.hitT[i] = h.t;
			buf.hitPath[i] = h.path;
			buf.hitN[i] = (uint8_t)h.nMajor;
			if( isHit ) atomicAdd( &buf.blockCount[i / CBLOCK], 1u ); // survivors per 256-path block (order-free count)
		}
		else if( kind == 1 )
		{
			buf.hitS[i] = isHit ? 1 : 0;
		}
		else
		{
			buf.hitE[i] = isHit ? 1 : 0;
			buf.hitEPath[i] = h.path;
		}
		dShadow += kind == 1 ? h.descents : 0u;
		dNormal += kind == 1 ? 0u : h.descents;
		nHits += ( kind != 1 && isHit ) ? 1u : 0u;
	}
};
template <int FL>
__global__ void __launch_bounds__( 64, MVRT_WAVES_OF( FL ) ) kPtTraceStream( PtParams P, TraceWorkspace ws, int stage, int setIdx, int nKinds, int shadowKind, uint32_t chunk,
																			uint32_t raysPerLane, uint32_t minWaves )
{
	PtIO io;
	io.table = P.buf.selfDev;
	io.setIdx = setIdx;
	io.n = P.buf.liveCount[stage];
	io.shadowKind = shadowKind;
	io.useHint = ( FL == 0 && stage > 0 && P.useHints ) ? 1 : 0;
	io.dNormal = io.dShadow = io.nHits = 0;
	const uint64_t total = (uint64_t)io.n * nKinds;
	// The grid is sized on the host for the upper bound (live counts stay on the device).  A launch with few rays is not throughput- but
	// latency-bound -- its time is the longest ray's iterations times the time of one iteration, and an iteration takes as long as the
	// SIMD's co-resident waves make it -- so it keeps only as many waves as give each lane raysPerLane rays (at least minWaves): fewer waves
	// per SIMD, each with its lanes refilled from a longer stretch of the stream.  The other workgroups retire at once.
	uint64_t nWaves = gridDim.x;
	if( raysPerLane )
	{
		uint64_t wantWaves = total / ( 64ull * raysPerLane ) + 1;
		if( wantWaves < minWaves ) wantWaves = minWaves;
		if( blockIdx.x >= wantWaves ) return;
		if( wantWaves < nWaves ) nWaves = wantWaves;
	}
	uint64_t c = total / ( nWaves * 4 );
	c = ( c + 63 ) / 64 * 64;
	if( c < 64 ) c = 64;
	if( c > chunk ) c = chunk;
	traceStream<FL>( makeTraceCore( P.svo ), io, total, P.buf.cursors + stage, (uint32_t)c, ws );
	unsigned long long dN = waveSum( (unsigned long long)io.dNormal ), dS = waveSum( (unsigned long long)io.dShadow ), nH = waveSum( (unsigned long long)io.nHits );
#ifdef MVRT_UTIL_STATS
	if( threadIdx.x == 0 )
	{
		atomicAdd( &P.buf.stats[8 + 0], io.utilIters );
		atomicAdd( &P.buf.stats[8 + 1], io.utilActive );
		atomicAdd( &P.buf.stats[8 + 2], io.utilTailIters );
		atomicAdd( &P.buf.stats[8 + 3], io.utilTailActive );
		atomicAdd( &P.buf.stats[12], io.utilRefillClocks );
		atomicAdd( &P.buf.stats[13], io.utilTotalClocks );
		atomicMax( &P.buf.stats[16 + stage], io.utilTailIters ); // longest-lived wave of the stage's launches, in node-visit iterations
		atomicAdd( &P.buf.stats[32 + stage], 1ull );			  // waves that worked
	}
	{
		unsigned long long m = io.utilMaxRayIters;
		for( int o = 32; o > 0; o >>= 1 )
		{
			const unsigned long long t = __shfl_xor( m, o );
			m = t > m ? t : m;
		}
		if( threadIdx.x == 0 ) atomicMax( &P.buf.stats[48 + stage], m ); // longest ray of the stage, in node-visit iterations
	}
#endif
	if( threadIdx.x == 0 )
	{
		if( dN ) atomicAdd( &P.buf.stats[2], dN );
		if( dS ) atomicAdd( &P.buf.stats[3], dS );
		if( nH ) atomicAdd( &P.buf.stats[4], nH );
	}
}

// ---- HDRI lookups (renderCommon.hpp:175-180,354-365,367-465) ---------------------------------------
MVRT_DI f3 hdriSampleNearest( const HdriDev& h, f3 d, bool isPrimary )
{
	int w = isPrimary ? h.widthPrimary : h.width;
	int hh = isPrimary ? h.heightPrimary : h.height;
	float phi = mvrt_atan2( d.z, d.x ) + MVRT_PI;
	float theta = mvrt_atan2( sqrtf( d.x * d.x + d.z * d.z ), d.y );
	float u = phi / ( MVRT_PI * 2.0f );
	float v = theta / MVRT_PI;
	int x = (int)smin( smax( u * w, 0.0f ), (float)( w - 1.0f ) );
	int y = (int)smin( smax( v * hh, 0.0f ), (float)( hh - 1.0f ) );
	uint64_t index = (uint64_t)y * w + x;
	const float4* px = ( isPrimary && h.pixelsPrimary ) ? h.pixelsPrimary : h.pixels;
	// no map loaded: only possible with the lighting switched off (scale 0: mvrt_pt_step refuses scale > 0 without a map), where a loaded map would
	// contribute pixel * 0 -- the reference reads m_pixels unconditionally here (voxKernel.cu:682) and its applications always load one
	if( !px ) return mk3( 0.0f, 0.0f, 0.0f );
	float4 c = px[index];
	return mk3( c.x, c.y, c.z ) * h.scale;
}
MVRT_DI uint32_t satH( const HdriDev& h, const uint32_t* s, uint32_t x ) { return x == 0 ? 0u : s[h.width * ( h.height - 1 ) + x - 1]; }
MVRT_DI uint32_t satV( const HdriDev& h, const uint32_t* s, uint32_t x, uint32_t y )
{
	if( y == 0 ) return 0u;
	uint32_t s0 = x == 0 ? 0u : s[h.width * ( y - 1 ) + ( x - 1 )];
	uint32_t s1 = s[h.width * ( y - 1 ) + x];
	return s1 - s0;
}
MVRT_DI uint32_t satCount( const HdriDev& h, const uint32_t* s, uint32_t x, uint32_t y )
{
	uint32_t a = ( x == 0 || y == 0 ) ? 0u : s[h.width * ( y - 1 ) + ( x - 1 )];
	uint32_t b = ( y == 0 ) ? 0u : s[h.width * ( y - 1 ) + x];
	uint32_t c = ( x == 0 ) ? 0u : s[h.width * y + ( x - 1 )];
	uint32_t d = s[h.width * y + x];
	return ( d - b ) + ( a - c );
}
MVRT_DI void hdriImportanceSample( const HdriDev& h, f3* dir, f3* L, float* pdf, f3 N, float u0, float u1, float u2, float u3 )
{
	const uint32_t* s = h.sat;
	uint32_t zero = h.zeroTables; // bit 0: the selected table is all zeros
	const float k = 0.8f;
	if( k < N.x ) s = h.sats[0], zero >>= 1;
	else if( N.x < -k ) s = h.sats[1], zero >>= 2;
	else if( k < N.y ) s = h.sats[2], zero >>= 3;
	else if( N.y < -k ) s = h.sats[3], zero >>= 4;
	else if( k < N.z ) s = h.sats[4], zero >>= 5;
	else if( N.z < -k ) s = h.sats[5], zero >>= 6;
	// Deviation from renderCommon.hpp:367-435: a table without a total > 0 selects nothing.  The reference would divide by vol == 0 and index about
	// 2^32 elements away.  L = 0, pdf = 1, dir = N: the NEE term is exactly 0, the shadow ray is still emitted (along N) and nothing is read.
	if( zero & 1u )
	{
		*dir = N;
		*L = mk3( 0.0f, 0.0f, 0.0f );
		*pdf = 1.0f;
		return;
	}

	int i = 0, j = h.width; // upper_bound_f, renderCommon.hpp:182-202
	while( i < j )
	{
		int m = ( i + j ) / 2;
		float value = (float)satH( h, s, m ) / 4294967296.0f; // (float)0xFFFFFFFFu
		if( value <= u0 ) i = m + 1;
		else j = m;
	}
	uint32_t X = (uint32_t)( i - 1 );
	uint32_t vol = satH( h, s, X + 1 ) - satH( h, s, X );
	i = 0;
	j = h.height;
	while( i < j )
	{
		int m = ( i + j ) / 2;
		float value = (float)satV( h, s, X, m ) / (float)vol;
		if( value <= u1 ) i = m + 1;
		else j = m;
	}
	uint32_t Y = (uint32_t)( i - 1 );
	float pSelection = (float)satCount( h, s, X, Y ) / 4294967296.0f;
	float dTheta = MVRT_PI / (float)h.height;
	float dPhi = 2.0f * MVRT_PI / (float)h.width;
	float theta = Y * dTheta;
	float dH = 2.0f * mvrt_sin( dTheta * 0.5f ) * mvrt_sin( dTheta * 0.5f + theta );
	float sr = dH * dPhi;
	float sY = mixf( mvrt_cos( theta ), mvrt_cos( theta + dTheta ), u2 );
	float phi = dPhi * ( (float)X + u3 ) + MVRT_PI;
	float sX, sZ;
	mvrt_sincos( phi, &sZ, &sX );
	float sinTheta = sqrtf( smax( 1.0f - sY * sY, 0.0f ) );
	*dir = mk3( sX * sinTheta, sY, sZ * sinTheta );
	*pdf = pSelection / sr;
	float4 color = h.pixels[Y * h.width + X];
	*L = mk3( color.x, color.y, color.z ) * h.scale;
}

// sampleLambertian + GetOrthonormalBasis, renderCommon.hpp:119-151
MVRT_DI f3 sampleLambertian( float a, float b, f3 Ng )
{
	float r = sqrtf( a );
	float theta = b * MVRT_PI * 2.0f;
	float sn, cs;
	mvrt_sincos( theta, &sn, &cs );
	float x = r * cs;
	float y = r * sn;
	float z = sqrtf( smax( 1.0f - a, 0.0f ) );
	const float sign = copysignf( 1.0f, Ng.z );
	const float aa = -1.0f / ( sign + Ng.z );
	const float bb = Ng.x * Ng.y * aa;
	f3 xaxis = mk3( 1.0f + sign * Ng.x * Ng.x * aa, sign * bb, -sign * Ng.x );
	f3 yaxis = mk3( bb, sign + Ng.y * Ng.y * aa, -Ng.y );
	return xaxis * x + yaxis * y + Ng * z;
}

MVRT_DI f3 voxelEmission( const SvoDev& s, uint32_t vIndex, bool withScale ) // IntersectorOctreeGPU.hpp:256-259
{
	return rawReflectance( s.attrs[vIndex].y ) * ( withScale ? s.emissionScale : 1.0f );
}

// ---- shade + compact: stage k consumes the hits of trace k, adds the contributions that became known,
// and for paths whose bounce ray hit, shades the hit (depth k of the reference loop, voxKernel.cu:691-760),
// writing the survivor to its STABLE compacted slot of the other PathSet. --------------------------------
#ifndef MVRT_SHADE_WAVES
#define MVRT_SHADE_WAVES 5 // waves per SIMD the shade kernel is register-budgeted for
#endif
// One-wave workgroups, no LDS, no barrier: a wave owns one 256-path block (CBLOCK and blockCount keep their meaning) and walks it as four 64-lane sub-blocks.
// The stable slot of a survivor is the block's scanned offset + the survivors of the earlier sub-blocks (a running scalar count) + its ballot rank.  One-wave
// workgroups find room beside the persistent traversal waves of the sibling pass, which hold all of a CU's LDS and most of its registers until their launch tail:
// the pipelined frame gains 1.0-1.5 % although the kernel alone is 12-18 % slower than the 256-thread form it replaces (profiles/r13_coresident_shade.txt).
template <int WAVES, class... ACTIVE> // WAVES = register budget: waves per SIMD the kernel is compiled for
__global__ void __launch_bounds__( WAVE, WAVES ) kPtShade( PtParams P, int stage, int inSet, ACTIVE... active )
{
	const uint64_t n = P.buf.liveCount[stage];
	const PathSet& in = P.buf.set[inSet];
	const PathSet& out = P.buf.set[inSet ^ 1];
	const bool lastStage = stage >= MVRT_MAX_DEPTH;
	const uint64_t nBlocks = ( n + CBLOCK - 1 ) / CBLOCK;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint32_t blockOffset = 0; // (nothing survives stage 8: no slots, and the counts stay as they are)
		if( !lastStage )
		{
			blockOffset = scanOffset( P.buf.blockCount, P.buf.tileBase, vb );
			if( threadIdx.x == 0 ) P.buf.blockCount[vb] = 0u; // the next stage's traversal counts its survivors into it again
		}
#pragma unroll 1
		for( uint64_t i = vb * CBLOCK + threadIdx.x; i < vb * CBLOCK + CBLOCK; i += WAVE ) // the four sub-blocks in turn (not unrolled: the body is ~2000 instructions)
		{
			if( i - threadIdx.x >= n ) break; // a sub-block past the end: uniform
			const bool valid = i < n;
			bool alive = false;
			uint32_t task = 0, vIndex = 0;
			uint2 attr = make_uint2( 0u, 0u );
			uint64_t hitPath = 0;
			int nMajor = 0;
			float t = MVRT_MAXF;
			f3 ro, rd, T, L;
			if( valid )
			{
				task = in.task[i];
				ro = mk3( in.rox[i], in.roy[i], in.roz[i] );
				rd = mk3( in.rdx[i], in.rdy[i], in.rdz[i] );
				t = P.buf.hitT[i];
				nMajor = P.buf.hitN[i];
				const bool hit = t != MVRT_MAXF;
				// the persistent traversal reports the hit voxel's path; its index is summed here, all lanes together
				hitPath = hit ? P.buf.hitPath[i] : 0ull;
				vIndex = hit ? voxelIndexFromPath( P.svo, hitPath ) : 0u;
				if( hit ) attr = P.svo.attrs[vIndex]; // colour and emission of the hit voxel: one 8-byte gather serves both uses below
				if( stage == 0 )
				{
					T = mk3( 1.0f, 1.0f, 1.0f );
					L = mk3( 0.0f, 0.0f, 0.0f );
					if( !hit ) // voxKernel.cu:678-684
					{
						L = L + T * hdriSampleNearest( P.hdri, rd, true );
					}
					else // :685-689
					{
						L = L + T * rawReflectance( attr.y ); // (IntersectorOctreeGPU.hpp:256-259 without the scale)
					}
				}
				else
				{
					T = mk3( in.Tx[i], in.Ty[i], in.Tz[i] );
					L = mk3( in.Lx[i], in.Ly[i], in.Lz[i] );
					if( P.hdriEnabled && P.buf.hitS[i] == 0 ) // :712-715, contribution computed when the ray was generated
					{
						L = L + mk3( in.nx[i], in.ny[i], in.nz[i] );
					}
					if( stage == 1 && P.extraSamples ) // :722-738
					{
						if( P.buf.hitE[i] )
						{
							const uint32_t ev = voxelIndexFromPath( P.svo, P.buf.hitEPath[i] );
							f3 Le = voxelEmission( P.svo, ev, true );
							L = L + T * Le / (float)( 1 + P.extraSamples );
						}
					}
					if( hit ) // :750-759
					{
						f3 Le = rawReflectance( attr.y ) * P.svo.emissionScale; // IntersectorOctreeGPU.hpp:256-259
						L = L + T * Le * ( stage == 1 ? 1.0f / (float)( 1 + P.extraSamples ) : 1.0f );
					}
				}
				alive = hit && !lastStage;
				if( !alive )
				{
					P.buf.Lsx[task] = L.x;
					P.buf.Lsy[task] = L.y;
					P.buf.Lsz[task] = L.z;
				}
			}
			if( lastStage ) continue; // nothing survives stage 8; uniform across the grid
			const unsigned long long aliveLanes = __ballot( alive );
			const uint32_t rank = __popcll( aliveLanes & ( ( 1ull << threadIdx.x ) - 1ull ) );
			const uint32_t slotBase = blockOffset; // first slot of this sub-block's survivors
			blockOffset += __popcll( aliveLanes );
			if( alive )
			{
				const uint64_t j = (uint64_t)slotBase + rank;
				// depth = stage of the reference loop
				uint32_t step, localPixel, localSpp;
				decodeTask( P.frame, task, &step, &localPixel, &localSpp );
				const uint32_t spp = ( P.frame.iteration + step ) * MVRT_SPP_PER_STEP + localSpp;
				const uint32_t stream = hashCombine2( 0u, globalPixel( P.frame, slotPixel( localPixel, active... ) ) );
				int dim = dimBase( stage, P.hdriEnabled, P.extraSamples );
				const f3 R = rawReflectance( attr.x ); // :693
				const f3 hitN = getHitN( nMajor, rd );				  // :694
				const f3 hitP = ro + rd * t;						  // :695
				f3 nee = mk3( 0.0f, 0.0f, 0.0f );
				if( P.hdriEnabled ) // :697-716
				{
					f2 u01 = pmjSample2d( P.pmj, spp, dim++, stream );
					f2 u23 = pmjSample2d( P.pmj, spp, dim++, stream );
					f3 sdir, emissive;
					float p;
					hdriImportanceSample( P.hdri, &sdir, &emissive, &p, hitN, u01.x, u01.y, u23.x, u23.y );
					nee = T * ( R / MVRT_PI ) * smax( dot3( hitN, sdir ), 0.0f ) * emissive / p;
					P.buf.sx[j] = sdir.x;
					P.buf.sy[j] = sdir.y;
					P.buf.sz[j] = sdir.z;
				}
				T = T * R;								// :718
				if( stage == 0 && P.extraSamples ) // :721-726
				{
					f2 u = pmjSample2d( P.pmj, spp, dim++, stream );
					f3 edir = sampleLambertian( u.x, u.y, hitN );
					P.buf.ex[j] = edir.x;
					P.buf.ey[j] = edir.y;
					P.buf.ez[j] = edir.z;
				}
				f2 u = pmjSample2d( P.pmj, spp, dim++, stream ); // :741-745
				f3 bdir = sampleLambertian( u.x, u.y, hitN );
				out.task[j] = task;
				if( P.svo.embedded ) out.org[j] = hintFromVoxelPath( hitPath, P.svo.levels ); // the rays of the next stage start on this voxel
				out.rox[j] = hitP.x;
				out.roy[j] = hitP.y;
				out.roz[j] = hitP.z;
				out.rdx[j] = bdir.x;
				out.rdy[j] = bdir.y;
				out.rdz[j] = bdir.z;
				out.Tx[j] = T.x;
				out.Ty[j] = T.y;
				out.Tz[j] = T.z;
				out.Lx[j] = L.x;
				out.Ly[j] = L.y;
				out.Lz[j] = L.z;
				out.nx[j] = nee.x;
				out.ny[j] = nee.y;
				out.nz[j] = nee.z;
			}
		}
	}
}

// ---- accumulate: frameBuffer[p].xyz += sum of the 16 samples in ascending spp order, .w += 16 -------
// (voxKernel.cu:763-774; the reference's LDS atomicAdd order is nondeterministic, ascending is ours)
// Masked: one thread per slot of the active list.  The reads of Ls* are those of the unmasked kernel (slot order, coalesced); the 16-byte read-modify-write of
// the pixel is scattered through the list, which ascends, so neighbouring lanes still touch neighbouring or identical cache lines.
template <class... ACTIVE>
__global__ void __launch_bounds__( 256 ) kPtAccumulate( PtParams P, float4* __restrict__ fb, ACTIVE... active )
{
	const uint64_t n = P.frame.validOwnedPixels;
	for( uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256 )
	{
		const uint64_t px = sizeof...( ACTIVE ) ? (uint64_t)slotPixel( (uint32_t)p, active... ) : p;
		float4 v = fb[px];
		for( int b = 0; b < P.frame.nSteps; b++ ) // merged steps are added one after the other, exactly as separate launches would
		{
			const uint64_t base = ( (uint64_t)b * n + p ) * MVRT_SPP_PER_STEP;
			const float4* sx = (const float4*)( P.buf.Lsx + base );
			const float4* sy = (const float4*)( P.buf.Lsy + base );
			const float4* sz = (const float4*)( P.buf.Lsz + base );
			float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll
			for( int q = 0; q < MVRT_SPP_PER_STEP / 4; q++ )
			{
				float4 vx = sx[q], vy = sy[q], vz = sz[q];
				ax += vx.x; ax += vx.y; ax += vx.z; ax += vx.w;
				ay += vy.x; ay += vy.y; ay += vy.z; ay += vy.w;
				az += vz.x; az += vz.y; az += vz.z; az += vz.w;
			}
			v.x += ax;
			v.y += ay;
			v.z += az;
			v.w += (float)MVRT_SPP_PER_STEP;
		}
		fb[px] = v;
	}
}

// ---- first-hit feature buffers (mvrt_pt_set_aovs) ----------------------------------------------------
// Runs right after the stage-0 traversal, when nothing is compacted yet: slot i == task i, so the 16 samples of (step, pixel) `ps` are entries
// ps * 16 .. ps * 16 + 15 of every array.  FOUR lanes per (step, pixel), lane q holding samples 4q .. 4q+3: every load is 16 bytes per lane (4 bytes of
// hitN) at consecutive addresses across the wave.  The 16 samples are added in ascending spp order starting from +0 like kPtAccumulate does: the running
// sum is handed from lane 0 to lane 3 of the group, each adding its four samples onto it in turn.  Writes, per (step, pixel), the partial sums
// { albedo.xyz, hits } and { normal.xyz, t } that kPtAovAccumulate adds to the buffers in step order.
struct AovRecords
{
	const float* hitT;
	const uint64_t* hitPath;
	const uint8_t* hitN;
	const float *rdx, *rdy, *rdz; // PathSet 0: the primary rays as kPtGenerate wrote them (stage 0 shades into set 1)
};
__global__ void __launch_bounds__( 256 ) kPtAovReduce( SvoDev svo, AovRecords r, uint64_t nPixelSteps, float4* __restrict__ partA, float4* __restrict__ partN )
{
	const uint32_t q = threadIdx.x & 3u;
	for( uint64_t ps = ( (uint64_t)blockIdx.x * 256 + threadIdx.x ) >> 2; ps < nPixelSteps; ps += (uint64_t)gridDim.x * 64 ) // (the 4 lanes of a group share ps)
	{
		const uint64_t base = ps * MVRT_SPP_PER_STEP + q * 4u;
		const float4 t4 = *(const float4*)( r.hitT + base );
		const ulonglong2 p01 = *(const ulonglong2*)( r.hitPath + base ), p23 = *(const ulonglong2*)( r.hitPath + base + 2 );
		const uint32_t n4 = *(const uint32_t*)( r.hitN + base );
		const float4 dx = *(const float4*)( r.rdx + base ), dy = *(const float4*)( r.rdy + base ), dz = *(const float4*)( r.rdz + base );
		const float t[4] = { t4.x, t4.y, t4.z, t4.w };
		const uint64_t path[4] = { p01.x, p01.y, p23.x, p23.y };
		const float rx[4] = { dx.x, dx.y, dx.z, dx.w }, ry[4] = { dy.x, dy.y, dy.z, dy.w }, rz[4] = { dz.x, dz.y, dz.z, dz.w };
		// the four gathers of this lane first (independent of the running sum), then the additions in order
		uint32_t colour[4];
#pragma unroll
		for( int k = 0; k < 4; k++ ) colour[k] = t[k] != MVRT_MAXF ? svo.attrs[voxelIndexFromPath( svo, path[k] )].x : 0u;
		float acc[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
		for( uint32_t turn = 0; turn < 4; turn++ )
		{
			if( q == turn )
			{
#pragma unroll
				for( int k = 0; k < 4; k++ )
				{
					if( t[k] == MVRT_MAXF ) continue; // a primary ray that missed adds nothing
					const f3 a = rawReflectance( colour[k] );
					const f3 n = getHitN( (int)( ( n4 >> ( 8 * k ) ) & 0xFFu ), mk3( rx[k], ry[k], rz[k] ) );
					acc[0] += a.x;
					acc[1] += a.y;
					acc[2] += a.z;
					acc[3] += 1.0f;
					acc[4] += n.x;
					acc[5] += n.y;
					acc[6] += n.z;
					acc[7] += t[k];
				}
			}
#pragma unroll
			for( int j = 0; j < 8; j++ ) acc[j] = __shfl( acc[j], (int)( ( threadIdx.x & 60u ) | turn ) ); // 4-lane groups never straddle a wave
		}
		if( q == 0 ) partA[ps] = make_float4( acc[0], acc[1], acc[2], acc[3] );
		if( q == 1 ) partN[ps] = make_float4( acc[4], acc[5], acc[6], acc[7] );
	}
}
// the partial sums of a pass, added to the two buffers one merged step after the other (launched behind kPtAccumulate: same event chain, same order)
// (masked: validOwnedPixels = the active pixels, the partial sums are indexed by slot and the two buffers through the list, as in kPtAccumulate)
template <class... ACTIVE>
__global__ void __launch_bounds__( 256 ) kPtAovAccumulate( uint64_t validOwnedPixels, int nSteps, const float4* __restrict__ partA, const float4* __restrict__ partN,
															 float4* __restrict__ albedo, float4* __restrict__ normalDepth, ACTIVE... active )
{
	for( uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < validOwnedPixels; p += (uint64_t)gridDim.x * 256 )
	{
		const uint64_t px = sizeof...( ACTIVE ) ? (uint64_t)slotPixel( (uint32_t)p, active... ) : p;
		float4 a = albedo[px], n = normalDepth[px];
		for( int b = 0; b < nSteps; b++ )
		{
			const float4 pa = partA[(uint64_t)b * validOwnedPixels + p], pn = partN[(uint64_t)b * validOwnedPixels + p];
			a.x += pa.x; a.y += pa.y; a.z += pa.z; a.w += pa.w;
			n.x += pn.x; n.y += pn.y; n.z += pn.z; n.w += pn.w;
		}
		albedo[px] = a;
		normalDepth[px] = n;
	}
}

// Grid of a path-tracer stage's traversal launch of `rays` rays (an upper bound: live counts stay on the device), and the small-launch limits the kernel applies
// to it (kPtTraceStream: raysPerLane, minWaves).  traceGridDiv = the frame's tile divisor.
struct PtTraceGrid
{
	int grid;
	uint32_t smallRpl, smallMinW;
};
static PtTraceGrid ptTraceGrid( uint64_t rays, int nCUs, int stage, int traceGridDiv )
{
	// a pass that shares the GPU with a sibling pass on another stream takes only 1/div of the wave slots, so that the two
	// really run side by side (a full persistent grid would hold every slot until its own tail)
	static const int envDiv = (int)mvrtKnob( "MVRT_TRACE_GRID_DIV", 0 );
	// ... for its BIG launches only (the first bounces; live counts are on the device, so the stage stands in for them): a small
	// launch finishes sooner the more lanes it may use, and is gone before it can be in the sibling's way
	static const int divMaxStage = (int)mvrtKnob( "MVRT_TRACE_DIV_MAX_STAGE", 99 );
	// small launches keep only total / (64 * 16) waves alive, at least 2048 (two per SIMD): measured with the 8-slot ring on a 1/8 tile
	// share -6.5 % (dragon, rtcamp stand-in), full frame -1 %, closed scene unchanged (gpurun_out/sweep_small2.log)
	static const uint32_t envRpl = (uint32_t)mvrtKnob( "MVRT_SMALL_RPL", 16 );
	static const uint32_t envMinW = (uint32_t)mvrtKnob( "MVRT_SMALL_MINW", 2048 );
	// experiment knob: waves per CU of a full-grid traversal launch (32 = every slot the register budget allows and then some)
	static const int wpc = (int)mvrtKnob( "MVRT_TRACE_WAVES_PER_CU", 0 );
	int g = streamGrid( rays, nCUs );
	const int div = stage > divMaxStage ? 1 : ( envDiv > 0 ? envDiv : traceGridDiv );
	if( div > 1 && g > nCUs * STREAM_WAVES_PER_CU / div ) g = nCUs * STREAM_WAVES_PER_CU / div;
	if( wpc > 0 && g > nCUs * wpc / ( div > 1 ? div : 1 ) ) g = nCUs * wpc / ( div > 1 ? div : 1 );
	return { g, envRpl, envMinW };
}

// Which build of the shade kernel a stage runs.
// Two builds of the kernel: stages 0 and 1 -- where most paths END (69 % of the primaries of an open scene miss) and the work per path is loads and a few adds --
// run the 8-waves-per-SIMD build (64 VGPRs, 44 bytes of scratch that the dying paths never touch); the deeper stages, whose paths mostly survive and run
// the ~2000-instruction shading, the 5-wave build.  r03, serial-mode shade time per 4 steps, stages {} / {0} / {0,1} / {1..8} / all on the 8-wave build:
// dragon 16.6 / 15.8 / 14.9 / 15.6 / 14.6 ms, closed cave 133.7 / 132.5 / 133.3 / 137.6 / 136.8 (tools/sweep_shade.sh)
static bool shadeDense8( int stage )
{
	static const int dense = (int)mvrtKnob( "MVRT_SHADE8_STAGES", 3 );
	return ( ( dense >> stage ) & 1 ) != 0;
}
// ... and the waves per CU of its grid.
// The grid-stride grids hold exactly the workgroups that are RESIDENT at once (8 / 5 per CU): r02 launched 8 per CU for the 5-wave build too, and the three
// that had to wait for a slot ran as a second, thin round -- most of what the 8-wave build seemed to gain.  5-wave build with 8 / 6 / 5 workgroups per CU:
// dragon 16.6 / 14.1 / 14.0 ms of shade time per 4 serial steps, cave 133.7 / 132.3 / 129.2
// (since the kernel holds no LDS its workgroups are single waves, each owning one 256-path block: the same 32 / 20 resident waves per CU as 32 / 20 workgroups)
static int shadeWavesPerCU( bool dense8 )
{
	static const int bpc8 = (int)mvrtKnob( "MVRT_SHADE_BPC8", 8 ), bpc5 = (int)mvrtKnob( "MVRT_SHADE_BPC5", 5 );
	return ( dense8 ? bpc8 : bpc5 ) * ( CBLOCK / WAVE );
}

// The masked instantiations are launched from functions defined BEHIND launchPtStep: a kernel template is emitted where it is first used, so every kernel of the
// unmasked path keeps the place in the code object that it has without the mask, and the masked ones follow them
static void launchMaskedGenerate( int grid, hipStream_t stream, const PtParams& P, const uint32_t* active );
static void launchMaskedShade( bool dense8, int grid, hipStream_t stream, const PtParams& P, int stage, int setIdx, const uint32_t* active );
static void launchMaskedAccumulate( int grid, hipStream_t stream, const PtParams& P, float4* frameBuffer, const AovBuffers* aov, const uint32_t* active );

int launchPtStep( const SvoDev& svo, const TraceWorkspace& ws, const HdriDev& hdri, const float2* pmj, const CameraPinhole* cams, const PtFrame& frame,
				  const PtBuffers& buf, float4* frameBuffer, int nCUs, PtProfiler* prof, hipStream_t stream, hipEvent_t accumulateAfter, const AovBuffers* aov, float4* moments,
				  const uint32_t* active )
{
	PtParams P;
	P.svo = svo;
	P.hdri = hdri;
	P.pmj = pmj;
	for( int b = 0; b < MVRT_MAX_BATCH; b++ ) P.cams[b] = cams[b < frame.nSteps ? b : 0];
	P.frame = frame;
	P.buf = buf;
	P.hdriEnabled = ( 0.0f < hdri.scale ) ? 1 : 0;
	P.extraSamples = svo.hasEmission ? 1 : 0;
	P.useHints = frame.useHints;
	if( nCUs <= 0 ) nCUs = numCUs();

	const uint64_t nSamples = frame.validOwnedPixels * MVRT_SPP_PER_STEP * frame.nSteps;
	if( nSamples == 0 ) return 0;
	if( nSamples * 3 >= 0xFFFFFFFFull )
	{
		mvrtSetError( "batch too large: %llu samples (ray indices are 32-bit)", (unsigned long long)nSamples );
		return 1;
	}
	if( nSamples > buf.cap )
	{
		mvrtSetError( "path buffers too small: %llu samples > capacity %llu", (unsigned long long)nSamples, (unsigned long long)buf.cap );
		return 1;
	}
	if( !ws.spill )
	{
		mvrtSetError( "internal: traversal workspace missing" );
		return 1;
	}

#define PROF_BEGIN( c ) if( prof ) prof->begin( c, stream )
#define PROF_END() if( prof ) prof->end( stream )

	PROF_BEGIN( MVRT_K_OTHER );
	if( active ) launchMaskedGenerate( persistentGrid( nSamples, 256, nCUs, 8 ), stream, P, active );
	else hipLaunchKernelGGL( kPtGenerate<>, dim3( persistentGrid( nSamples, 256, nCUs, 8 ) ), dim3( 256 ), 0, stream, P );
	PROF_END();

	for( int stage = 0; stage <= MVRT_MAX_DEPTH; stage++ )
	{
		const int setIdx = stage & 1;
		const int shadowKind = ( stage > 0 && P.hdriEnabled ) ? 1 : 0;
		const int extraKind = ( stage == 1 && P.extraSamples ) ? 1 : 0;
		const int nKinds = 1 + shadowKind + extraKind;
		PROF_BEGIN( MVRT_K_TRACE );
		{
			const PtTraceGrid tg = ptTraceGrid( nSamples * nKinds, nCUs, stage, frame.traceGridDiv );
			withFlavour( svo, [&]( auto fl ) {
				hipLaunchKernelGGL( kPtTraceStream<decltype( fl )::value>, dim3( tg.grid ), dim3( 64 ), 0, stream, P, ws, stage, setIdx, nKinds, shadowKind, streamChunk( nSamples * nKinds, tg.grid ),
									tg.smallRpl, tg.smallMinW );
			} );
		}
		PROF_END();
		if( aov && stage == 0 ) // the first-hit records are complete and still in task order; the stage-1 traversal overwrites them, the stage-1 shade the directions
		{
			const AovRecords rec = { buf.hitT, buf.hitPath, buf.hitN, buf.set[0].rdx, buf.set[0].rdy, buf.set[0].rdz };
			const uint64_t nPixelSteps = frame.validOwnedPixels * frame.nSteps;
			PROF_BEGIN( MVRT_K_OTHER );
			hipLaunchKernelGGL( kPtAovReduce, dim3( persistentGrid( nPixelSteps * 4, 256, nCUs, 8 ) ), dim3( 256 ), 0, stream, svo, rec, nPixelSteps, aov->partA, aov->partN );
			PROF_END();
		}
		PROF_BEGIN( MVRT_K_OTHER );
		// survivors per block were counted by the traversal's result stores; scan them (and account the rays).  One-wave workgroups without LDS: they find a
		// wave slot on a CU whose LDS the traversal waves of a sibling pass hold
		launchScan( buf.blockCount, buf.tileBase, nSamples, (const uint32_t*)( buf.liveCount + stage ), stage < MVRT_MAX_DEPTH ? buf.liveCount + stage + 1 : (uint32_t*)nullptr, buf.stats,
					nKinds, shadowKind, stream );
		PROF_END();
		PROF_BEGIN( MVRT_K_SHADE );
		{
			const bool dense8 = shadeDense8( stage );
			const int wpc = shadeWavesPerCU( dense8 );
			if( active ) launchMaskedShade( dense8, persistentGrid( nSamples, CBLOCK, nCUs, wpc ), stream, P, stage, setIdx, active );
			else if( dense8 )
				hipLaunchKernelGGL( kPtShade<8>, dim3( persistentGrid( nSamples, CBLOCK, nCUs, wpc ) ), dim3( WAVE ), 0, stream, P, stage, setIdx );
			else
				hipLaunchKernelGGL( kPtShade<MVRT_SHADE_WAVES>, dim3( persistentGrid( nSamples, CBLOCK, nCUs, wpc ) ), dim3( WAVE ), 0, stream, P, stage, setIdx );
		}
		PROF_END();
		if( buf.dbgTasks && stage < MVRT_MAX_DEPTH ) // debug capture: the compacted survivor list this stage wrote (parity of the compaction indices)
			MVRT_HIP( hipMemcpyAsync( buf.dbgTasks + (uint64_t)stage * buf.cap, buf.set[setIdx ^ 1].task, nSamples * 4, hipMemcpyDeviceToDevice, stream ) );
	}
	// frame-buffer additions must happen in step order (fixed fp32 summation order): wait for the previous step's
	if( accumulateAfter ) MVRT_HIP( hipStreamWaitEvent( stream, accumulateAfter, 0 ) );
	PROF_BEGIN( MVRT_K_OTHER );
	if( active ) launchMaskedAccumulate( persistentGrid( frame.validOwnedPixels, 256, nCUs, 8 ), stream, P, frameBuffer, nullptr, active );
	else hipLaunchKernelGGL( kPtAccumulate<>, dim3( persistentGrid( frame.validOwnedPixels, 256, nCUs, 8 ) ), dim3( 256 ), 0, stream, P, frameBuffer );
	PROF_END();
	if( aov )
	{
		PROF_BEGIN( MVRT_K_OTHER );
		if( active ) launchMaskedAccumulate( persistentGrid( frame.validOwnedPixels, 256, nCUs, 8 ), stream, P, nullptr, aov, active );
		else
			hipLaunchKernelGGL( kPtAovAccumulate<>, dim3( persistentGrid( frame.validOwnedPixels, 256, nCUs, 8 ) ), dim3( 256 ), 0, stream, frame.validOwnedPixels, frame.nSteps, aov->partA,
								aov->partN, aov->albedo, aov->normalDepth );
		PROF_END();
	}
	if( moments ) // luminance moments (mvrt_pt_set_moments): the Ls* planes are complete until the next pass of this slot generates
	{
		PROF_BEGIN( MVRT_K_OTHER );
		const int rc = launchPtMoments( buf, frame.validOwnedPixels, frame.nSteps, moments, nCUs, stream, active );
		PROF_END();
		if( rc ) return rc;
	}
	MVRT_HIP( hipGetLastError() );
	return 0;
}

static void launchMaskedGenerate( int grid, hipStream_t stream, const PtParams& P, const uint32_t* active )
{
	hipLaunchKernelGGL( kPtGenerate<const uint32_t*>, dim3( grid ), dim3( 256 ), 0, stream, P, active );
}
static void launchMaskedShade( bool dense8, int grid, hipStream_t stream, const PtParams& P, int stage, int setIdx, const uint32_t* active )
{
	if( dense8 ) hipLaunchKernelGGL( ( kPtShade<8, const uint32_t*> ), dim3( grid ), dim3( WAVE ), 0, stream, P, stage, setIdx, active );
	else hipLaunchKernelGGL( ( kPtShade<MVRT_SHADE_WAVES, const uint32_t*> ), dim3( grid ), dim3( WAVE ), 0, stream, P, stage, setIdx, active );
}
// frameBuffer: the frame-buffer addition; aov: that of the two feature buffers
static void launchMaskedAccumulate( int grid, hipStream_t stream, const PtParams& P, float4* frameBuffer, const AovBuffers* aov, const uint32_t* active )
{
	if( frameBuffer ) hipLaunchKernelGGL( kPtAccumulate<const uint32_t*>, dim3( grid ), dim3( 256 ), 0, stream, P, frameBuffer, active );
	if( aov )
		hipLaunchKernelGGL( kPtAovAccumulate<const uint32_t*>, dim3( grid ), dim3( 256 ), 0, stream, P.frame.validOwnedPixels, P.frame.nSteps, aov->partA, aov->partN, aov->albedo,
							aov->normalDepth, active );
}
