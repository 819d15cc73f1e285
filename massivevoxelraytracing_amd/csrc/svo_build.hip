// svo_build.hip -- IntersectorOctreeGPU::build on the GPU (reference IntersectorOctreeGPU.hpp:40-241 with
// kernels voxKernel.cu:58-435), redesigned so that the result is DETERMINISTIC and numbered exactly
// like the CPU reference builder buildOctreeDAGReference (IntersectorOctree.hpp:11-123):
//
//   voxelize (six-separating, Schwarz-Seidel; voxelization.hpp:124-337)   [kVoxCount, kVoxelize]
//   radix sort (morton, attribute) pairs                                   [rocPRIM via hipCUB; replaces tinyhipradixsort]
//   unique with integer-mean attributes (voxKernel.cu:170-243)             [head flags -> stable compaction -> kUniqueEmit]
//   one octree level per pass, bottom-up (voxKernel.cu:269-424):
//       group <=8 siblings -> candidate node {mask, children[8], nVoxelsPSum[8]}
//       DAG de-duplication WITHOUT the reference's racy CAS hash table: 64-bit content hash,
//       stable radix sort of (hash, group), equal-content runs collapse onto their FIRST group,
//       new node index = rank of that first occurrence in group order = creation order of the
//       CPU reference (std::map find-or-insert while walking groups in morton order).
//   embed child masks into child pointers (voxKernel.cu:426-435)
//
// All fp32 arithmetic of the voxelizer is contraction-free and matches the oracle bit for bit.
#include <hipcub/hipcub.hpp>

#include <utility>
#include <vector>

#include "launch.h"

#define WAVE 64
#define BB 256

namespace
{
// ---------------------------------------------------------------------------------------------------
// voxelizer (voxelization.hpp:124-337), six-separating only -- the GPU reference hard-codes it
// (voxKernel.cu:68,109)
// ---------------------------------------------------------------------------------------------------
struct i2
{
	int x, y;
};
MVRT_DI void proj2( f3 p, int axis, float* a, float* b ) // project2plane, voxelization.hpp:15-34
{
	if( axis == 0 ) { *a = p.x; *b = p.y; }
	else if( axis == 1 ) { *a = p.y; *b = p.z; }
	else { *a = p.z; *b = p.x; }
}
MVRT_DI float projRem( f3 p, int axis ) { return axis == 0 ? p.z : ( axis == 1 ? p.x : p.y ); } // :36-48
MVRT_DI void proj2i( int x, int y, int z, int axis, int* a, int* b )
{
	if( axis == 0 ) { *a = x; *b = y; }
	else if( axis == 1 ) { *a = y; *b = z; }
	else { *a = z; *b = x; }
}
MVRT_DI int projRemI( int x, int y, int z, int axis ) { return axis == 0 ? z : ( axis == 1 ? x : y ); }
MVRT_DI f3 cross3( f3 a, f3 b ) { return mk3( a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x ); }

// float -> int of the voxelizer as the reference's HOST build performs it (x86 cvttss2si: NaN and everything outside [-2^31, 2^31) give INT_MIN).  The
// hardware conversion gives 0 for NaN and saturates instead, which made a triangle with a zero normal (two equal vertices: kx, ky NaN) emit the voxels
// of z index 0 of its bounding box where the reference and the oracle emit none (tests/test_gpu_reference_pins.py).
MVRT_DI int f2iHost( float f ) { return ( f >= -2147483648.0f && f < 2147483648.0f ) ? (int)f : (int)0x80000000u; }

struct VT
{
	int major;
	int lox, loy, hix, hiy, loz, hiz;
	float dC[3][3], nX[3][3], nY[3][3];
	float ox, oy, oz;
	float kx, ky, cSix, cMax, cMin;
	bool conservative; // voxelization.hpp's sixSeparating == false: every voxel the triangle touches (:186-189, :296-301)

	MVRT_DI void init( f3 v0, f3 v1, f3 v2, f3 origin, float dps, int gridRes, bool conservativeMode = false ) // :148-229
	{
		conservative = conservativeMode;
		f3 e01 = v1 - v0;
		f3 e12 = v2 - v1;
		f3 n = cross3( e01, e12 );
		{
			float x = sabs( n.x ), y = sabs( n.y ), z = sabs( n.z ); // majorAxis, :84-94
			major = ( x < y ) ? ( y < z ? 0 : 2 ) : ( x < z ? 0 : 1 );
		}
		f3 bl = mk3( smin( smin( v0.x, v1.x ), v2.x ), smin( smin( v0.y, v1.y ), v2.y ), smin( smin( v0.z, v1.z ), v2.z ) );
		f3 bu = mk3( smax( smax( v0.x, v1.x ), v2.x ), smax( smax( v0.y, v1.y ), v2.y ), smax( smax( v0.z, v1.z ), v2.z ) );
		int lx = f2iHost( floorf( ( bl.x - origin.x ) / dps ) ), ly = f2iHost( floorf( ( bl.y - origin.y ) / dps ) ), lz = f2iHost( floorf( ( bl.z - origin.z ) / dps ) );
		int ux = f2iHost( floorf( ( bu.x - origin.x ) / dps ) ), uy = f2iHost( floorf( ( bu.y - origin.y ) / dps ) ), uz = f2iHost( floorf( ( bu.z - origin.z ) / dps ) );
		lx = lx < 0 ? 0 : lx;
		ly = ly < 0 ? 0 : ly;
		lz = lz < 0 ? 0 : lz;
		ux = ux > gridRes - 1 ? gridRes - 1 : ux;
		uy = uy > gridRes - 1 ? gridRes - 1 : uy;
		uz = uz > gridRes - 1 ? gridRes - 1 : uz;
		proj2i( lx, ly, lz, major, &lox, &loy );
		proj2i( ux, uy, uz, major, &hix, &hiy );
		loz = projRemI( lx, ly, lz, major );
		hiz = projRemI( ux, uy, uz, major );
#pragma unroll
		for( int axis = 0; axis < 3; axis++ )
		{
			float ax[3], ay[3];
			proj2( v0, axis, &ax[0], &ay[0] );
			proj2( v1, axis, &ax[1], &ay[1] );
			proj2( v2, axis, &ax[2], &ay[2] );
			float rem = projRem( n, axis );
			float nSign = 0.0f < rem ? 1.0f : -1.0f;
#pragma unroll
			for( int edge = 0; edge < 3; edge++ )
			{
				int e1 = ( edge + 1 ) % 3;
				float ex = ax[e1] - ax[edge], ey = ay[e1] - ay[edge];
				float nex = -ey * nSign, ney = ex * nSign;
				nX[axis][edge] = nex;
				nY[axis][edge] = ney;
				if( conservative ) // max(ne.x*dp.x, 0) + max(ne.y*dp.y, 0) - dot(ne, a)   (:186-189)
				{
					dC[axis][edge] = smax( nex * dps, 0.0f ) + smax( ney * dps, 0.0f ) - ( nex * ax[edge] + ney * ay[edge] );
				}
				else // six-separating: dot(ne, dp*0.5 - a) + 0.5*dps*max(|ne.x|,|ne.y|)   (:190-193)
				{
					float hx = dps * 0.5f - ax[edge], hy = dps * 0.5f - ay[edge];
					dC[axis][edge] = ( nex * hx + ney * hy ) + 0.5f * dps * smax( sabs( nex ), sabs( ney ) );
				}
			}
		}
		proj2( origin, major, &ox, &oy );
		oz = projRem( origin, major );
		float v0x, v0y;
		proj2( v0, major, &v0x, &v0y );
		float v0z = projRem( v0, major );
		float nx, ny;
		proj2( n, major, &nx, &ny );
		float nz = projRem( n, major );
		kx = -nx / nz;
		ky = -ny / nz;
		float K = -kx * v0x - ky * v0y + v0z;
		cMax = K + dps * ( smax( kx, 0.0f ) + smax( ky, 0.0f ) ); // :225-227
		cMin = K + dps * ( smin( kx, 0.0f ) + smin( ky, 0.0f ) );
		cSix = K + 0.5f * dps * ( kx + ky );
	}
	MVRT_DI i2 yRange( int x, float dps ) const // :235-274
	{
		float xcoord = ox + x * dps;
		float miny = -3.402823466e+38F, maxy = 3.402823466e+38F;
		for( int edge = 0; edge < 3; edge++ )
		{
			float nex = nX[major][edge], ney = nY[major][edge], d = dC[major][edge];
			if( ney == 0.0f )
			{
				if( -nex * xcoord <= d ) continue;
				return i2{ 1, -1 };
			}
			float k = -( xcoord * nex + d ) / ney;
			if( 0.0f < ney ) miny = smax( miny, k );
			else maxy = smin( maxy, k );
		}
		float minIndexF = smax( ( miny - oy ) / dps, -2147483648.0f );
		float maxIndexF = smin( ( maxy - oy ) / dps, 2147483520.0f );
		int lowerY = f2iHost( ceilf( minIndexF ) );
		int upperY = f2iHost( floorf( maxIndexF ) );
		lowerY = lowerY < loy ? loy : lowerY;
		upperY = upperY > hiy ? hiy : upperY;
		return i2{ lowerY, upperY };
	}
	MVRT_DI i2 zRange( int x, int y, float dps ) const // :275-306
	{
		float px = ox + dps * x, py = oy + dps * y;
		float var = kx * px + ky * py;
		int zmin, zmax;
		if( conservative ) // :296-301
		{
			float tmax = var + cMax, tmin = var + cMin;
			zmin = f2iHost( floorf( ( tmin - oz ) / dps ) );
			zmax = f2iHost( floorf( ( tmax - oz ) / dps ) );
		}
		else
		{
			float tsix = var + cSix;
			float indexf = ( tsix - oz ) / dps;
			float zf = floorf( indexf );
			int z = f2iHost( zf );
			zmin = indexf == zf ? (int)( (uint32_t)z - 1u ) : z; // (z = INT_MIN wraps like the host build, the range is empty either way)
			zmax = z;
		}
		zmin = zmin < loz ? loz : zmin;
		zmax = zmax > hiz ? hiz : zmax;
		return i2{ zmin, zmax };
	}
	MVRT_DI f3 point( int x, int y, int z, float dps ) const // :307-312 + unProjectPlane :96-108
	{
		float a = ox + dps * x, b = oy + dps * y, r = oz + (float)z * dps;
		return major == 0 ? mk3( a, b, r ) : ( major == 1 ? mk3( r, a, b ) : mk3( b, r, a ) );
	}
	MVRT_DI bool intersect( f3 p ) const // :318-336
	{
		if( loz == hiz ) return true;
		for( int axis = 0; axis < 3; axis++ )
		{
			if( axis == major ) continue;
			float a, b;
			proj2( p, axis, &a, &b );
			for( int edge = 0; edge < 3; edge++ )
			{
				float d = nX[axis][edge] * a + nY[axis][edge] * b + dC[axis][edge];
				if( d < 0.0f ) return false;
			}
		}
		return true;
	}
};

MVRT_DI f3 loadV( const float* p, uint64_t i ) { return mk3( p[i * 3], p[i * 3 + 1], p[i * 3 + 2] ); }

// closestBarycentricCoordinateOnTriangle, vectorMath.hpp:249-284
MVRT_DI f3 closestBary( f3 v0, f3 v1, f3 v2, f3 P )
{
	f3 d0 = v0 - P, d1 = v1 - P, d2 = v2 - P;
	f3 e0 = v2 - v0, e1 = v0 - v1, e2 = v1 - v2;
	f3 Ng = cross3( e2, e0 );
	float U = dot3( cross3( d2, d0 ), Ng );
	float V = dot3( cross3( d0, d1 ), Ng );
	float W = dot3( cross3( d1, d2 ), Ng );
	if( U < 0.0f )
	{
		V = dot3( mk3( -d0.x, -d0.y, -d0.z ), e0 );
		W = dot3( d2, e0 );
	}
	else if( V < 0.0f )
	{
		W = dot3( mk3( -d1.x, -d1.y, -d1.z ), e1 );
		U = dot3( d0, e1 );
	}
	else if( W < 0.0f )
	{
		U = dot3( mk3( -d2.x, -d2.y, -d2.z ), e2 );
		V = dot3( d1, e2 );
	}
	f3 bc = mk3( smax( 0.0f, U ), smax( 0.0f, V ), smax( 0.0f, W ) );
	return bc / ( bc.x + bc.y + bc.z );
}

// voxCount (EMIT = false, voxKernel.cu:58-90) and voxelize (EMIT = true, :91-166) share one body.
// The reference gives every triangle one thread, whatever its size; a wall of two triangles across a 4096^3 grid is then 16.7 M cell tests on ONE lane (seconds,
// with 63 lanes of its wave and the rest of the chip idle).  Here a lane only does its own triangle when its footprint is small; triangles whose projected bounding
// rectangle exceeds VOX_BIG_CELLS cells are done by the whole WAVE afterwards, one after the other, the columns of the footprint dealt to the 64 lanes.  Which lane
// emits which voxel -- and so the order of the dumped list -- differs from the reference's; nothing downstream depends on it: the list is sorted by Morton code and the
// attributes of duplicates are integer sums (voxKernel.cu:194-220).
#define VOX_BIG_CELLS 2048
MVRT_DI uint32_t voxColumns( const VT& c, float dps, int x0, int xStep, bool emit, f3 v0, f3 v1, f3 v2, f3 c0, f3 c1, f3 c2, f3 e0, f3 e1, f3 e2, uint64_t* __restrict__ mortonOut,
							 uint64_t* __restrict__ attrOut, uint64_t dst )
{
	uint32_t k = 0;
	for( int x = x0; x <= c.hix; x += xStep )
	{
		i2 yr = c.yRange( x, dps );
		for( int y = yr.x; y <= yr.y; y++ )
		{
			i2 zr = c.zRange( x, y, dps );
			for( int z = zr.x; z <= zr.y; z++ )
			{
				f3 p = c.point( x, y, z, dps );
				if( !c.intersect( p ) ) continue;
				if( emit )
				{
					int cx, cy, cz; // VTContext::i -> unProjectPlane, :110-122,313-316
					if( c.major == 0 ) { cx = x; cy = y; cz = z; }
					else if( c.major == 1 ) { cx = z; cy = x; cz = y; }
					else { cx = y; cy = z; cz = x; }
					mortonOut[dst + k] = mortonEncode( cx, cy, cz );
					f3 bc = closestBary( v0, v1, v2, p );
					f3 bColor = c1 * bc.x + c2 * bc.y + c0 * bc.z;	 // bc.x * c1 + bc.y * c2 + bc.z * c0, voxKernel.cu:148
					f3 bEmission = e1 * bc.x + e2 * bc.y + e0 * bc.z; // :149
					uint64_t a = (uint64_t)(uint8_t)( bColor.x * 255.0f + 0.5f ) | (uint64_t)(uint8_t)( bColor.y * 255.0f + 0.5f ) << 8 |
								 (uint64_t)(uint8_t)( bColor.z * 255.0f + 0.5f ) << 16 | 255ull << 24 | (uint64_t)(uint8_t)( bEmission.x * 255.0f + 0.5f ) << 32 |
								 (uint64_t)(uint8_t)( bEmission.y * 255.0f + 0.5f ) << 40 | (uint64_t)(uint8_t)( bEmission.z * 255.0f + 0.5f ) << 48 | 255ull << 56;
					attrOut[dst + k] = a;
				}
				k++;
			}
		}
	}
	return k;
}
template <bool EMIT>
__global__ void __launch_bounds__( 128 ) kVoxelize( const float* __restrict__ verts, const float* __restrict__ cols, const float* __restrict__ emis, uint32_t nTri,
													 unsigned long long* counter, f3 origin, float dps, int gridRes, uint64_t* __restrict__ mortonOut,
													 uint64_t* __restrict__ attrOut, int conservative )
{
	const uint32_t iTri = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	const f3 white = mk3( 1, 1, 1 ), black = mk3( 0, 0, 0 ); // voxUtil.hpp:49-61 defaults
	bool big = false;
	if( iTri < nTri )
	{
		f3 v0 = loadV( verts, (uint64_t)iTri * 3 ), v1 = loadV( verts, (uint64_t)iTri * 3 + 1 ), v2 = loadV( verts, (uint64_t)iTri * 3 + 2 );
		VT c;
		c.init( v0, v1, v2, origin, dps, gridRes, conservative != 0 );
		big = (long long)( c.hix - c.lox + 1 ) * (long long)( c.hiy - c.loy + 1 ) > VOX_BIG_CELLS;
		if( !big )
		{
			const uint32_t nVoxels = voxColumns( c, dps, c.lox, 1, false, v0, v1, v2, white, white, white, black, black, black, nullptr, nullptr, 0 );
			if( !EMIT )
			{
				if( nVoxels ) atomicAdd( counter, (unsigned long long)nVoxels );
			}
			else if( nVoxels )
			{
				const uint64_t dst = atomicAdd( counter, (unsigned long long)nVoxels );
				f3 c0 = white, c1 = white, c2 = white, e0 = black, e1 = black, e2 = black;
				if( cols )
				{
					c0 = loadV( cols, (uint64_t)iTri * 3 );
					c1 = loadV( cols, (uint64_t)iTri * 3 + 1 );
					c2 = loadV( cols, (uint64_t)iTri * 3 + 2 );
				}
				if( emis )
				{
					e0 = loadV( emis, (uint64_t)iTri * 3 );
					e1 = loadV( emis, (uint64_t)iTri * 3 + 1 );
					e2 = loadV( emis, (uint64_t)iTri * 3 + 2 );
				}
				voxColumns( c, dps, c.lox, 1, true, v0, v1, v2, c0, c1, c2, e0, e1, e2, mortonOut, attrOut, dst );
			}
		}
	}
	// ---- the big triangles of this wave, one after the other, by all 64 lanes (every lane of the wave reaches this point) ----
	unsigned long long todo = __ballot( big );
	while( todo )
	{
		const uint32_t src = (uint32_t)__builtin_ctzll( todo );
		todo &= todo - 1ull;
		const uint32_t t = ( blockIdx.x * blockDim.x + ( threadIdx.x & ~63u ) ) + src; // the triangle of lane `src` of this wave
		f3 v0 = loadV( verts, (uint64_t)t * 3 ), v1 = loadV( verts, (uint64_t)t * 3 + 1 ), v2 = loadV( verts, (uint64_t)t * 3 + 2 );
		VT c;
		c.init( v0, v1, v2, origin, dps, gridRes, conservative != 0 );
		const uint32_t mine = voxColumns( c, dps, c.lox + (int)lane, 64, false, v0, v1, v2, white, white, white, black, black, black, nullptr, nullptr, 0 );
		uint32_t incl = mine; // inclusive prefix over the lanes
		for( int o = 1; o < 64; o <<= 1 )
		{
			const uint32_t up = __shfl_up( incl, o, 64 );
			if( (int)lane >= o ) incl += up;
		}
		const uint32_t total = __shfl( incl, 63, 64 );
		if( total == 0 ) continue;
		unsigned long long base = 0;
		if( lane == 0 ) base = atomicAdd( counter, (unsigned long long)total );
		if( !EMIT ) continue;
		base = (unsigned long long)__shfl( (uint32_t)base, 0, 64 ) | ( (unsigned long long)__shfl( (uint32_t)( base >> 32 ), 0, 64 ) << 32 );
		f3 c0 = white, c1 = white, c2 = white, e0 = black, e1 = black, e2 = black;
		if( cols )
		{
			c0 = loadV( cols, (uint64_t)t * 3 );
			c1 = loadV( cols, (uint64_t)t * 3 + 1 );
			c2 = loadV( cols, (uint64_t)t * 3 + 2 );
		}
		if( emis )
		{
			e0 = loadV( emis, (uint64_t)t * 3 );
			e1 = loadV( emis, (uint64_t)t * 3 + 1 );
			e2 = loadV( emis, (uint64_t)t * 3 + 2 );
		}
		voxColumns( c, dps, c.lox + (int)lane, 64, true, v0, v1, v2, c0, c1, c2, e0, e1, e2, mortonOut, attrOut, base + ( incl - mine ) );
	}
}

// ---------------------------------------------------------------------------------------------------
// stable compaction helpers (same scheme as kernels_rt.hip: count per 256 -> scan -> rank)
// ---------------------------------------------------------------------------------------------------
template <class Pred>
MVRT_DI void countBody( Pred pred, uint64_t n, uint32_t* __restrict__ blockCount )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * BB + threadIdx.x;
		bool keep = i < n ? pred( i ) : false;
		unsigned long long b = __ballot( keep );
		if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) wc[threadIdx.x / WAVE] = __popcll( b );
		__syncthreads();
		if( threadIdx.x == 0 ) blockCount[vb] = wc[0] + wc[1] + wc[2] + wc[3];
		__syncthreads();
	}
}
MVRT_DI uint32_t rankInBlock( bool keep, uint32_t* wc )
{
	unsigned long long b = __ballot( keep );
	uint32_t lane = threadIdx.x & ( WAVE - 1 ), w = threadIdx.x / WAVE;
	uint32_t inWave = __popcll( b & ( ( 1ull << lane ) - 1ull ) );
	if( lane == 0 ) wc[w] = __popcll( b );
	__syncthreads();
	uint32_t off = 0;
	for( uint32_t k = 0; k < w; k++ ) off += wc[k];
	__syncthreads();
	return off + inWave;
}
__global__ void __launch_bounds__( 1024 ) kScanCounts( uint32_t* __restrict__ blockCount, uint64_t nItems, uint32_t* __restrict__ totalOut )
{
	__shared__ uint32_t part[1024];
	uint32_t nBlocks = (uint32_t)( ( nItems + BB - 1 ) / BB );
	uint32_t per = ( nBlocks + 1023 ) / 1024;
	uint32_t beg = threadIdx.x * per;
	uint32_t end = beg + per < nBlocks ? beg + per : nBlocks;
	uint32_t sum = 0;
	for( uint32_t i = beg; i < end; i++ ) sum += blockCount[i];
	part[threadIdx.x] = sum;
	__syncthreads();
	for( uint32_t off = 1; off < 1024; off <<= 1 )
	{
		uint32_t v = part[threadIdx.x];
		if( threadIdx.x >= off ) v += part[threadIdx.x - off];
		__syncthreads();
		part[threadIdx.x] = v;
		__syncthreads();
	}
	uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
	for( uint32_t i = beg; i < end; i++ )
	{
		uint32_t c = blockCount[i];
		blockCount[i] = run;
		run += c;
	}
	if( threadIdx.x == 1023 ) *totalOut = part[1023];
}

// ---- unique (voxKernel.cu:170-243) ---------------------------------------------------------------------
__global__ void __launch_bounds__( BB ) kUniqueCount( const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ blockCount )
{
	countBody( [=]( uint64_t i ) { return i == 0 || keys[i - 1] != keys[i]; }, n, blockCount );
}
__global__ void __launch_bounds__( BB ) kUniqueEmit( const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, uint64_t n, const uint32_t* __restrict__ blockOff,
													  uint64_t* __restrict__ keysOut, uint2* __restrict__ attrsOut, uint32_t* __restrict__ hasEmission )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * BB + threadIdx.x;
		bool head = i < n ? ( i == 0 || keys[i - 1] != keys[i] ) : false;
		uint32_t r = rankInBlock( head, wc );
		if( head )
		{
			uint64_t morton = keys[i];
			int s[6] = { 0, 0, 0, 0, 0, 0 };
			int cnt = 0;
			for( uint64_t j = i; j < n && keys[j] == morton; j++ ) // :201-210 integer sums
			{
				uint64_t a = vals[j];
				s[0] += (int)( a & 0xFF );
				s[1] += (int)( ( a >> 8 ) & 0xFF );
				s[2] += (int)( ( a >> 16 ) & 0xFF );
				s[3] += (int)( ( a >> 32 ) & 0xFF );
				s[4] += (int)( ( a >> 40 ) & 0xFF );
				s[5] += (int)( ( a >> 48 ) & 0xFF );
				cnt++;
			}
			uint32_t col = (uint32_t)( s[0] / cnt ) | (uint32_t)( s[1] / cnt ) << 8 | (uint32_t)( s[2] / cnt ) << 16 | 255u << 24;
			uint32_t em = (uint32_t)( s[3] / cnt ) | (uint32_t)( s[4] / cnt ) << 8 | (uint32_t)( s[5] / cnt ) << 16 | 255u << 24;
			uint64_t dst = (uint64_t)blockOff[vb] + r;
			keysOut[dst] = morton;
			attrsOut[dst] = make_uint2( col, em );
			if( em & 0xFFFFFFu ) atomicOr( hasEmission, 1u ); // :225-228
		}
	}
}

// ---- octree levels ---------------------------------------------------------------------------------------
struct Task // OctreeTask, voxCommon.hpp:29-36
{
	uint64_t morton;
	uint32_t child;
	uint32_t count;
};
struct Cand // candidate node of one sibling group
{
	uint32_t children[8];
	uint32_t psum[8];
	uint32_t mask;
	uint32_t total;
};

__global__ void __launch_bounds__( BB ) kInitTasks( const uint64_t* __restrict__ morton, uint32_t n, Task* __restrict__ tasks )
{
	for( uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BB )
	{
		Task t;
		t.morton = morton[i];
		t.child = MVRT_LEAF; // octreeTaskInit, voxKernel.cu:253-255
		t.count = 1;
		tasks[i] = t;
	}
}
__global__ void __launch_bounds__( BB ) kGroupCount( const Task* __restrict__ tasks, uint64_t n, uint32_t* __restrict__ blockCount )
{
	countBody( [=]( uint64_t i ) { return i == 0 || ( tasks[i - 1].morton >> 3 ) != ( tasks[i].morton >> 3 ); }, n, blockCount );
}

MVRT_HDI uint64_t mix64( uint64_t h, uint64_t k )
{
	k *= 0x87c37b91114253d5ull;
	k = ( k << 31 ) | ( k >> 33 );
	k *= 0x4cf5ad432745937full;
	h ^= k;
	h = ( h << 27 ) | ( h >> 37 );
	return h * 5 + 0x52dce729ull;
}
MVRT_HDI uint64_t fmix64( uint64_t k )
{
	k ^= k >> 33;
	k *= 0xff51afd7ed558ccdull;
	k ^= k >> 33;
	k *= 0xc4ceb9fe1a85ec53ull;
	k ^= k >> 33;
	return k;
}

// one thread per sibling group head: gather <= 8 tasks into a candidate node (voxKernel.cu:293-320)
__global__ void __launch_bounds__( BB ) kMakeCandidates( const Task* __restrict__ tasks, uint64_t n, const uint32_t* __restrict__ blockOff, Cand* __restrict__ cands,
														  uint64_t* __restrict__ hashes, uint32_t* __restrict__ groupIds, uint64_t* __restrict__ parentMorton )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * BB + threadIdx.x;
		bool head = i < n ? ( i == 0 || ( tasks[i - 1].morton >> 3 ) != ( tasks[i].morton >> 3 ) ) : false;
		uint32_t r = rankInBlock( head, wc );
		if( head )
		{
			Cand c;
			for( int j = 0; j < 8; j++ )
			{
				c.children[j] = MVRT_LEAF;
				c.psum[j] = 0;
			}
			c.mask = 0;
			uint64_t parent = tasks[i].morton >> 3;
			for( uint64_t j = i; j < n && ( tasks[j].morton >> 3 ) == parent; j++ )
			{
				Task t = tasks[j];
				uint32_t space = (uint32_t)( t.morton & 7 );
				c.mask |= 1u << space;
				c.children[space] = t.child;
				c.psum[space] = t.count;
			}
			uint32_t run = 0;
			for( int j = 0; j < 8; j++ ) // exclusive prefix sum, :313-320
			{
				uint32_t v = c.psum[j];
				c.psum[j] = run;
				run += v;
			}
			c.total = run;
			uint32_t g = blockOff[vb] + r;
			cands[g] = c;
			uint64_t h = mix64( 0x9e3779b97f4a7c15ull, c.mask );
			for( int j = 0; j < 8; j += 2 ) h = mix64( h, (uint64_t)c.children[j] | (uint64_t)c.children[j + 1] << 32 );
			hashes[g] = fmix64( h );
			groupIds[g] = g;
			parentMorton[g] = parent;
		}
	}
}

MVRT_DI bool sameContent( const Cand& a, const Cand& b ) // OctreeNode::operator==, voxCommon.hpp:147-161
{
	if( a.mask != b.mask ) return false;
	for( int j = 0; j < 8; j++ )
		if( a.children[j] != b.children[j] ) return false;
	return true;
}

// in hash-sorted order: run head = first element whose (hash, content) differs from its predecessor.
// headPos[i] = i for heads, 0 otherwise (an inclusive max-scan then gives each element its run head).
__global__ void __launch_bounds__( BB ) kMarkRuns( const uint64_t* __restrict__ sortedHash, const uint32_t* __restrict__ sortedGroup, const Cand* __restrict__ cands, uint32_t n,
													uint32_t* __restrict__ headPos )
{
	for( uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BB )
	{
		bool head = i == 0 || sortedHash[i] != sortedHash[i - 1] || !sameContent( cands[sortedGroup[i]], cands[sortedGroup[i - 1]] );
		headPos[i] = head ? (uint32_t)i : 0u;
	}
}
// repOf[group] = first (smallest) group of its equal-content run; the sort is stable and groups entered it
// in ascending order, so the run head carries the smallest group id
__global__ void __launch_bounds__( BB ) kScatterReps( const uint32_t* __restrict__ sortedGroup, const uint32_t* __restrict__ headPosScanned, uint32_t n,
													   uint32_t* __restrict__ repOf )
{
	for( uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BB )
	{
		repOf[sortedGroup[i]] = sortedGroup[headPosScanned[i]];
	}
}
__global__ void __launch_bounds__( BB ) kIdentityReps( uint32_t n, uint32_t* __restrict__ repOf )
{
	for( uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BB ) repOf[i] = (uint32_t)i;
}
__global__ void __launch_bounds__( BB ) kFirstCount( const uint32_t* __restrict__ repOf, uint64_t n, uint32_t* __restrict__ blockCount )
{
	countBody( [=]( uint64_t g ) { return repOf[g] == (uint32_t)g; }, n, blockCount );
}
// first occurrences get node index nodeBase + rank (creation order); they also write the node
__global__ void __launch_bounds__( BB ) kEmitNodes( const uint32_t* __restrict__ repOf, const Cand* __restrict__ cands, uint64_t n, const uint32_t* __restrict__ blockOff,
													 uint32_t nodeBase, Node64* __restrict__ nodes, uint8_t* __restrict__ masks, uint32_t* __restrict__ nodeOfGroup )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t g = vb * BB + threadIdx.x;
		bool first = g < n ? repOf[g] == (uint32_t)g : false;
		uint32_t r = rankInBlock( first, wc );
		if( first )
		{
			uint32_t idx = nodeBase + blockOff[vb] + r;
			const Cand& c = cands[g];
			Node64 nd;
			for( int j = 0; j < 8; j++ )
			{
				nd.children[j] = c.children[j];
				nd.psum[j] = c.psum[j];
			}
			nodes[idx] = nd;
			masks[idx] = (uint8_t)c.mask;
			nodeOfGroup[g] = idx;
		}
	}
}
__global__ void __launch_bounds__( BB ) kNextTasks( const uint32_t* __restrict__ repOf, const uint32_t* __restrict__ nodeOfGroup, const Cand* __restrict__ cands,
													 const uint64_t* __restrict__ parentMorton, uint32_t n, Task* __restrict__ tasksOut )
{
	for( uint64_t g = (uint64_t)blockIdx.x * BB + threadIdx.x; g < n; g += (uint64_t)gridDim.x * BB )
	{
		Task t;
		t.morton = parentMorton[g];
		t.child = nodeOfGroup[repOf[g]];
		t.count = cands[g].total;
		tasksOut[g] = t;
	}
}
// embedMasks, voxKernel.cu:426-435 / voxCommon.hpp:183-195
__global__ void __launch_bounds__( BB ) kEmbedMasks( Node64* __restrict__ nodes, const uint8_t* __restrict__ masks, uint32_t nNodes )
{
	uint64_t gid = (uint64_t)blockIdx.x * BB + threadIdx.x;
	uint64_t node = gid / 8;
	uint32_t k = gid % 8;
	if( node >= nNodes ) return;
	uint32_t child = nodes[node].children[k];
	if( child == MVRT_LEAF ) return;
	nodes[node].children[k] = child | (uint32_t)masks[child] << 24;
}

// ---- no-DAG path: every sibling group becomes a node, written straight to its final slot (group index = node index
// within the level; the reference's ENABLE_GPU_DAG-off branch, voxKernel.cu:322-334, numbers them with a racing
// atomicInc -- here the numbering is the deterministic group order) ------------------------------------------------------
__global__ void __launch_bounds__( BB ) kMakeNodesDirect( const Task* __restrict__ tasks, uint64_t n, const uint32_t* __restrict__ blockOff, uint32_t nodeBase,
														   Node64* __restrict__ nodes, uint8_t* __restrict__ masks, Task* __restrict__ tasksOut )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * BB + threadIdx.x;
		bool head = i < n ? ( i == 0 || ( tasks[i - 1].morton >> 3 ) != ( tasks[i].morton >> 3 ) ) : false;
		uint32_t r = rankInBlock( head, wc );
		if( head )
		{
			Node64 nd;
			for( int j = 0; j < 8; j++ )
			{
				nd.children[j] = MVRT_LEAF;
				nd.psum[j] = 0;
			}
			uint32_t mask = 0;
			const uint64_t parent = tasks[i].morton >> 3;
			for( uint64_t j = i; j < n && ( tasks[j].morton >> 3 ) == parent; j++ )
			{
				Task t = tasks[j];
				uint32_t space = (uint32_t)( t.morton & 7 );
				mask |= 1u << space;
				nd.children[space] = t.child;
				nd.psum[space] = t.count;
			}
			uint32_t run = 0;
			for( int j = 0; j < 8; j++ )
			{
				uint32_t v = nd.psum[j];
				nd.psum[j] = run;
				run += v;
			}
			const uint32_t g = blockOff[vb] + r;
			const uint64_t idx = (uint64_t)nodeBase + g;
			nodes[idx] = nd;
			masks[idx] = (uint8_t)mask;
			Task o;
			o.morton = parent;
			o.child = (uint32_t)idx;
			o.count = run;
			tasksOut[g] = o;
		}
	}
}
// ---- "tree" flavour (no DAG and too many nodes for embedded masks, or embedding switched off): the nodes are never materialised as 64-byte
// lines.  In a tree built level by level in morton order the children of a node are CONSECUTIVE nodes of the level below, so a node is
// { mask, index of its first child } (5 bytes; for the parents of voxels: index of their first voxel), and what the traversal reads are
// BRICKS: one 16-byte record per node of every second level { the masks of its 8 children, its own mask, where the children of its first
// child start } (four bricks share a 64-byte line) -- one fetch advances the traversal TWO levels (traverse_stream.h, flavour 2). ------------
__global__ void __launch_bounds__( BB ) kMakeNodesTree( const Task* __restrict__ tasks, uint64_t n, const uint32_t* __restrict__ blockOff, uint32_t nodeBase, int bottomLevel,
														 uint8_t* __restrict__ cMask, uint32_t* __restrict__ cFirst, Task* __restrict__ tasksOut )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		uint64_t i = vb * BB + threadIdx.x;
		bool head = i < n ? ( i == 0 || ( tasks[i - 1].morton >> 3 ) != ( tasks[i].morton >> 3 ) ) : false;
		uint32_t r = rankInBlock( head, wc );
		if( head )
		{
			uint32_t mask = 0, run = 0;
			const uint64_t parent = tasks[i].morton >> 3;
			for( uint64_t j = i; j < n && ( tasks[j].morton >> 3 ) == parent; j++ )
			{
				mask |= 1u << (uint32_t)( tasks[j].morton & 7 );
				run += tasks[j].count;
			}
			const uint32_t g = blockOff[vb] + r;
			const uint64_t idx = (uint64_t)nodeBase + g;
			cMask[idx] = (uint8_t)mask;
			cFirst[idx] = bottomLevel ? (uint32_t)i : tasks[i].child; // first voxel (= its vIndex) / first child node: the rest follow consecutively
			Task o;
			o.morton = parent;
			o.child = (uint32_t)idx;
			o.count = run;
			tasksOut[g] = o;
		}
	}
}
// bricks of one (odd) builder level: node r = levelBase + g has children k = cFirst[r] + j in the level below.  grandBase / grandBrickBase
// translate the children's first-child indices (nodes two levels below) into brick indices; childIsBottom: the children are parents of voxels
// and their cFirst already IS a voxel index.
__global__ void __launch_bounds__( BB ) kMakeBricks( const uint8_t* __restrict__ cMask, const uint32_t* __restrict__ cFirst, uint32_t levelBase, uint32_t count, int childIsBottom,
													  uint32_t grandBase, uint32_t grandBrickBase, uint4* __restrict__ bricksOfLevel )
{
	for( uint64_t g = (uint64_t)blockIdx.x * BB + threadIdx.x; g < count; g += (uint64_t)gridDim.x * BB )
	{
		const uint32_t r = levelBase + (uint32_t)g;
		const uint32_t mask = cMask[r];
		uint32_t k = cFirst[r];
		uint32_t lo = 0, hi = 0, base = 0;
		bool first = true;
		for( int c = 0; c < 8; c++ )
		{
			if( mask >> c & 1u )
			{
				const uint32_t m = cMask[k];
				if( first ) base = childIsBottom ? cFirst[k] : grandBrickBase + ( cFirst[k] - grandBase );
				first = false;
				if( c < 4 ) lo |= m << ( 8 * c );
				else hi |= m << ( 8 * ( c - 4 ) );
				k++;
			}
		}
		// A brick is 16 bytes: the masks of the root's eight children (byte c = child c, 0 = absent), the root's own mask, and where the children
		// of its first existing child start (bricks two levels down, or voxels).  The children of consecutive nodes lie back to back -- every level
		// is numbered in Morton order -- so child c's start is base + popcount( child masks before c ): nothing else of the brick is ever read
		// (traverse_stream.h, treeDescend), and the up to eight bricks below one node share 128 bytes.
		bricksOfLevel[g] = make_uint4( lo, hi, mask, base );
	}
}
// distinct parents per level for ALL levels in one pass (the reference's octreeTaskInit counters, voxKernel.cu:257-265)
__global__ void __launch_bounds__( BB ) kLevelCounts( const uint64_t* __restrict__ morton, uint64_t n, int levels, unsigned long long* __restrict__ counts )
{
	// per-workgroup tallies in LDS, one global atomic per level and workgroup at the end (13 hot addresses took 0.64 s of global
	// atomics for 650 M voxels when every wave added to them directly)
	__shared__ unsigned int tally[32];
	if( threadIdx.x < 32 ) tally[threadIdx.x] = 0u;
	__syncthreads();
	for( uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BB )
	{
		const uint64_t a = morton[i], b = i ? morton[i - 1] : 0;
		for( int l = 0; l < levels; l++ )
		{
			const bool head = i == 0 || ( a >> ( 3 * ( l + 1 ) ) ) != ( b >> ( 3 * ( l + 1 ) ) );
			const unsigned long long m = __ballot( head );
			if( head && ( threadIdx.x & 63 ) == (uint32_t)__builtin_ctzll( m ) ) atomicAdd( &tally[l], (unsigned int)__popcll( m ) );
		}
	}
	__syncthreads();
	if( threadIdx.x < (uint32_t)levels && tally[threadIdx.x] ) atomicAdd( &counts[threadIdx.x], (unsigned long long)tally[threadIdx.x] );
}
// seeded synthetic voxels: uniformly random cells of the grid with hash-derived colours; ~1/256 of them emissive
MVRT_HDI uint64_t splitmix64( uint64_t x )
{
	x += 0x9E3779B97F4A7C15ull;
	x = ( x ^ ( x >> 30 ) ) * 0xBF58476D1CE4E5B9ull;
	x = ( x ^ ( x >> 27 ) ) * 0x94D049BB133111EBull;
	return x ^ ( x >> 31 );
}
__global__ void __launch_bounds__( BB ) kSyntheticVoxels( uint64_t n, uint64_t seed, uint32_t gridRes, uint64_t* __restrict__ mortonOut, uint64_t* __restrict__ attrOut )
{
	for( uint64_t i = (uint64_t)blockIdx.x * BB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BB )
	{
		const uint64_t h = splitmix64( seed + i );
		const uint64_t c = splitmix64( h );
		const uint32_t x = (uint32_t)( h ) & ( gridRes - 1 ), y = (uint32_t)( h >> 21 ) & ( gridRes - 1 ), z = (uint32_t)( h >> 42 ) & ( gridRes - 1 );
		mortonOut[i] = mortonEncode( x, y, z );
		const uint64_t rgb = ( ( c & 0xFFFFFFull ) | 0x404040ull ); // keep reflectance above 0.25
		const uint64_t emissive = ( ( c >> 56 ) == 0 ) ? rgb : 0ull;
		attrOut[i] = rgb | 255ull << 24 | emissive << 32 | 255ull << 56;
	}
}

// ---- voxel lists: build from xyz, batched edits (mvrt_svo_build_voxels / _edit_voxels; the read-back of _read_voxels is kWalkGather, kernels_walk.hip) ----------------
// encode + validate: xyz (3 x u32) + VoxelAttirb (NULL = white, no emission) -> (Morton, attribute with both alphas 255).  ENC_PER entries per thread: 48 bytes of
// coordinates = three 16-byte loads (vec: the caller's arrays are 16-byte aligned).  firstBad[0] / [1]: lowest entry outside the grid / with an op byte other than
// MVRT_VOXEL_REMOVE (0) or MVRT_VOXEL_SET (1), one atomicMin per wave.  idxOut (edits): the batch index, the value of the stable sort that follows.
#define ENC_PER 4
MVRT_DI void store2( uint64_t* p, uint64_t a, uint64_t b ) { *(uint4*)p = make_uint4( (uint32_t)a, (uint32_t)( a >> 32 ), (uint32_t)b, (uint32_t)( b >> 32 ) ); }
__global__ void __launch_bounds__( BB ) kEncodeVoxels( const uint32_t* __restrict__ xyz, const uint32_t* __restrict__ attribs, const uint8_t* __restrict__ ops, uint64_t n, uint32_t gridRes,
														int vec, uint64_t* __restrict__ keysOut, uint64_t* __restrict__ valsOut, uint32_t* __restrict__ idxOut,
														unsigned long long* __restrict__ firstBad )
{
	const uint64_t nQuads = ( n + ENC_PER - 1 ) / ENC_PER;
	const uint64_t nBlocks = ( nQuads + BB - 1 ) / BB;
	const uint32_t lane = threadIdx.x & ( WAVE - 1 );
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		const uint64_t q = vb * BB + threadIdx.x;
		const uint64_t i0 = q * ENC_PER;
		const int cnt = q < nQuads ? (int)( n - i0 < ENC_PER ? n - i0 : ENC_PER ) : 0;
		uint32_t c[ENC_PER * 3] = {}, a[ENC_PER * 2] = {};
		if( vec && cnt == ENC_PER )
		{
			const uint4* p = (const uint4*)( xyz + i0 * 3 );
			const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
			c[0] = v0.x; c[1] = v0.y; c[2] = v0.z; c[3] = v0.w; c[4] = v1.x; c[5] = v1.y;
			c[6] = v1.z; c[7] = v1.w; c[8] = v2.x; c[9] = v2.y; c[10] = v2.z; c[11] = v2.w;
			if( attribs )
			{
				const uint4* pa = (const uint4*)( attribs + i0 * 2 );
				const uint4 w0 = pa[0], w1 = pa[1];
				a[0] = w0.x; a[1] = w0.y; a[2] = w0.z; a[3] = w0.w; a[4] = w1.x; a[5] = w1.y; a[6] = w1.z; a[7] = w1.w;
			}
		}
		else
		{
#pragma unroll
			for( int k = 0; k < ENC_PER; k++ )
			{
				if( k >= cnt ) continue;
				c[3 * k] = xyz[( i0 + k ) * 3];
				c[3 * k + 1] = xyz[( i0 + k ) * 3 + 1];
				c[3 * k + 2] = xyz[( i0 + k ) * 3 + 2];
				if( attribs )
				{
					a[2 * k] = attribs[( i0 + k ) * 2];
					a[2 * k + 1] = attribs[( i0 + k ) * 2 + 1];
				}
			}
		}
		if( !attribs )
		{
#pragma unroll
			for( int k = 0; k < ENC_PER; k++ )
			{
				a[2 * k] = 0xFFFFFFFFu; // white (voxUtil.hpp:49-61)
				a[2 * k + 1] = 0u;		// no emission
			}
		}
		uint64_t bad = ~0ull, badOp = ~0ull, key[ENC_PER], val[ENC_PER];
#pragma unroll
		for( int k = 0; k < ENC_PER; k++ )
		{
			const uint64_t i = i0 + k;
			const uint32_t x = c[3 * k], y = c[3 * k + 1], z = c[3 * k + 2];
			if( k < cnt && ( x >= gridRes || y >= gridRes || z >= gridRes ) && bad == ~0ull ) bad = i;
			if( k < cnt && ops && ops[i] > 1u && badOp == ~0ull ) badOp = i;
			key[k] = k < cnt ? mortonEncode( x, y, z ) : 0;
			val[k] = (uint64_t)( a[2 * k] | 0xFF000000u ) | (uint64_t)( a[2 * k + 1] | 0xFF000000u ) << 32;
		}
		if( cnt == ENC_PER )
		{
			store2( keysOut + i0, key[0], key[1] );
			store2( keysOut + i0 + 2, key[2], key[3] );
			store2( valsOut + i0, val[0], val[1] );
			store2( valsOut + i0 + 2, val[2], val[3] );
			if( idxOut ) *(uint4*)( idxOut + i0 ) = make_uint4( (uint32_t)i0, (uint32_t)i0 + 1, (uint32_t)i0 + 2, (uint32_t)i0 + 3 );
		}
		else
		{
#pragma unroll
			for( int k = 0; k < ENC_PER; k++ )
			{
				if( k >= cnt ) continue;
				keysOut[i0 + k] = key[k];
				valsOut[i0 + k] = val[k];
				if( idxOut ) idxOut[i0 + k] = (uint32_t)( i0 + k );
			}
		}
		// lanes hold ascending index ranges: the lowest lane with a bad entry has the wave's lowest
		unsigned long long m = __ballot( bad != ~0ull );
		if( m && lane == (uint32_t)__builtin_ctzll( m ) ) atomicMin( &firstBad[0], (unsigned long long)bad );
		m = __ballot( badOp != ~0ull );
		if( m && lane == (uint32_t)__builtin_ctzll( m ) ) atomicMin( &firstBad[1], (unsigned long long)badOp );
	}
}

MVRT_DI uint2 asAttr( uint64_t v ) { return make_uint2( (uint32_t)v, (uint32_t)( v >> 32 ) ); }

enum EditKind : uint8_t
{
	EDIT_NOOP = 0,	  // REMOVE of an absent voxel
	EDIT_INSERT = 1,  // SET of an absent voxel
	EDIT_REPLACE = 2, // SET of an existing voxel
	EDIT_REMOVE = 3	  // REMOVE of an existing voxel
};
// edits sorted by (Morton, batch index): the LAST entry of each key survives
__global__ void __launch_bounds__( BB ) kEditTailCount( const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ blockCount )
{
	countBody( [=]( uint64_t k ) { return k + 1 == n || keys[k + 1] != keys[k]; }, n, blockCount );
}
// survivors -> the sorted unique edit list, each classified against the old sorted voxel list (binary search: pos = its rank among the old codes).
// eInc = (insert, removal) as the low / high word, exclusively scanned afterwards; counts[0..2] = inserts, removals, replacements
__global__ void __launch_bounds__( BB ) kEditClassify( const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n, const uint32_t* __restrict__ blockOff,
														const uint64_t* __restrict__ attrN, const uint8_t* __restrict__ ops, const uint64_t* __restrict__ oldMorton, uint32_t nOld,
														uint64_t* __restrict__ eKeys, uint64_t* __restrict__ eAttr, uint32_t* __restrict__ ePos, uint8_t* __restrict__ eKind,
														unsigned long long* __restrict__ eInc, uint32_t* __restrict__ counts )
{
	__shared__ uint32_t wc[BB / WAVE];
	const uint64_t nBlocks = ( n + BB - 1 ) / BB;
	const uint32_t lane = threadIdx.x & ( WAVE - 1 );
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		const uint64_t k = vb * BB + threadIdx.x;
		const bool tail = k < n ? ( k + 1 == n || keys[k + 1] != keys[k] ) : false;
		const uint32_t r = rankInBlock( tail, wc );
		uint32_t kind = EDIT_NOOP;
		if( tail )
		{
			const uint64_t key = keys[k];
			const uint32_t j = idx[k];
			const uint32_t op = ops ? ops[j] : 1u;
			const uint64_t pos = lowerBound( oldMorton, 0, nOld, key );
			const bool found = pos < nOld && oldMorton[pos] == key;
			kind = op ? ( found ? EDIT_REPLACE : EDIT_INSERT ) : ( found ? EDIT_REMOVE : EDIT_NOOP );
			const uint64_t e = (uint64_t)blockOff[vb] + r;
			eKeys[e] = key;
			eAttr[e] = attrN[j];
			ePos[e] = (uint32_t)pos;
			eKind[e] = (uint8_t)kind;
			eInc[e] = ( kind == EDIT_INSERT ? 1ull : 0ull ) | ( kind == EDIT_REMOVE ? 1ull << 32 : 0ull );
		}
		const unsigned long long mi = __ballot( tail && kind == EDIT_INSERT ), mr = __ballot( tail && kind == EDIT_REMOVE ), mp = __ballot( tail && kind == EDIT_REPLACE );
		if( lane == 0 )
		{
			if( mi ) atomicAdd( &counts[0], (uint32_t)__popcll( mi ) );
			if( mr ) atomicAdd( &counts[1], (uint32_t)__popcll( mr ) );
			if( mp ) atomicAdd( &counts[2], (uint32_t)__popcll( mp ) );
		}
	}
}
// structural edit, old side: one streaming pass over the old (Morton, attribute) arrays, MERGE_PER voxels per thread with 16-byte loads.  Old voxel i lands at
// i + (inserts before it) - (removals before it), both read from the scanned edit list at e = lower_bound( edits, its code ); the edits a block of voxels can meet
// lie between the bounds of its first and last code (the common case: none, and no lane searches).
#define MERGE_PER 2
__global__ void __launch_bounds__( BB ) kMergeOld( const uint64_t* __restrict__ oldMorton, const uint2* __restrict__ oldAttrs, uint32_t nOld, const uint64_t* __restrict__ eKeys,
													const uint64_t* __restrict__ eAttr, const uint8_t* __restrict__ eKind, const unsigned long long* __restrict__ ePre, uint32_t nE,
													uint64_t* __restrict__ newMorton, uint2* __restrict__ newAttrs, uint32_t* __restrict__ hasEmission )
{
	__shared__ uint32_t range[2];
	const uint64_t per = (uint64_t)BB * MERGE_PER;
	const uint64_t nBlocks = ( nOld + per - 1 ) / per;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		const uint64_t b0 = vb * per, b1 = b0 + per < nOld ? b0 + per : nOld;
		if( threadIdx.x == 0 )
		{
			range[0] = (uint32_t)lowerBound( eKeys, 0, nE, oldMorton[b0] );
			range[1] = (uint32_t)lowerBound( eKeys, range[0], nE, oldMorton[b1 - 1] );
		}
		__syncthreads();
		const uint64_t lo = range[0], hi = range[1];
		__syncthreads();
		const uint64_t i = b0 + (uint64_t)threadIdx.x * MERGE_PER;
		bool em = false;
		if( i < b1 )
		{
			uint64_t m[MERGE_PER];
			uint2 a[MERGE_PER];
			const int cnt = i + 1 < b1 ? 2 : 1;
			if( cnt == 2 )
			{
				const uint4 mm = *(const uint4*)( oldMorton + i );
				const uint4 aa = *(const uint4*)( oldAttrs + i );
				m[0] = (uint64_t)mm.x | (uint64_t)mm.y << 32;
				m[1] = (uint64_t)mm.z | (uint64_t)mm.w << 32;
				a[0] = make_uint2( aa.x, aa.y );
				a[1] = make_uint2( aa.z, aa.w );
			}
			else
			{
				m[0] = oldMorton[i];
				a[0] = oldAttrs[i];
				m[1] = 0;
				a[1] = make_uint2( 0, 0 );
			}
#pragma unroll
			for( int k = 0; k < MERGE_PER; k++ )
			{
				if( k >= cnt ) continue;
				const uint64_t e = lo == hi ? lo : lowerBound( eKeys, lo, hi, m[k] );
				const uint32_t kind = e < nE && eKeys[e] == m[k] ? eKind[e] : (uint32_t)EDIT_NOOP;
				if( kind == EDIT_REMOVE ) continue;
				const uint2 at = kind == EDIT_REPLACE ? asAttr( eAttr[e] ) : a[k];
				const unsigned long long p = ePre[e];
				const uint64_t out = i + k + (uint32_t)p - (uint32_t)( p >> 32 );
				newMorton[out] = m[k];
				newAttrs[out] = at;
				em |= ( at.y & 0xFFFFFFu ) != 0u;
			}
		}
		if( __ballot( em ) && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicOr( hasEmission, 1u );
	}
}
// structural edit, insert side: insert e lands after the old voxels below it (ePos) minus the removals and plus the inserts before it
__global__ void __launch_bounds__( BB ) kMergeInserts( const uint64_t* __restrict__ eKeys, const uint64_t* __restrict__ eAttr, const uint8_t* __restrict__ eKind,
														const uint32_t* __restrict__ ePos, const unsigned long long* __restrict__ ePre, uint32_t nE, uint64_t* __restrict__ newMorton,
														uint2* __restrict__ newAttrs, uint32_t* __restrict__ hasEmission )
{
	for( uint64_t e = (uint64_t)blockIdx.x * BB + threadIdx.x; e < nE; e += (uint64_t)gridDim.x * BB )
	{
		if( eKind[e] != EDIT_INSERT ) continue;
		const unsigned long long p = ePre[e];
		const uint64_t out = (uint64_t)ePos[e] + (uint32_t)p - (uint32_t)( p >> 32 );
		const uint2 at = asAttr( eAttr[e] );
		newMorton[out] = eKeys[e];
		newAttrs[out] = at;
		if( at.y & 0xFFFFFFu ) atomicOr( hasEmission, 1u );
	}
}
// attribute-only edit: new attributes in place (vIndex = Morton rank does not move), then hasEmission of the whole set again (it can turn either way)
__global__ void __launch_bounds__( BB ) kScatterAttrs( const uint64_t* __restrict__ eAttr, const uint8_t* __restrict__ eKind, const uint32_t* __restrict__ ePos, uint32_t nE,
														uint2* __restrict__ attrs )
{
	for( uint64_t e = (uint64_t)blockIdx.x * BB + threadIdx.x; e < nE; e += (uint64_t)gridDim.x * BB )
		if( eKind[e] == EDIT_REPLACE ) attrs[ePos[e]] = asAttr( eAttr[e] );
}
__global__ void __launch_bounds__( BB ) kAnyEmission( const uint2* __restrict__ attrs, uint32_t n, uint32_t* __restrict__ hasEmission )
{
	const uint64_t nPairs = ( (uint64_t)n + 1 ) / 2;
	const uint64_t nBlocks = ( nPairs + BB - 1 ) / BB;
	for( uint64_t vb = blockIdx.x; vb < nBlocks; vb += gridDim.x )
	{
		const uint64_t i = ( vb * BB + threadIdx.x ) * 2;
		bool em = false;
		if( i + 1 < n )
		{
			const uint4 aa = *(const uint4*)( attrs + i );
			em = ( ( aa.y | aa.w ) & 0xFFFFFFu ) != 0u;
		}
		else if( i < n )
			em = ( attrs[i].y & 0xFFFFFFu ) != 0u;
		if( __ballot( em ) && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) atomicOr( hasEmission, 1u );
	}
}
struct MaxOp
{
	__host__ __device__ uint32_t operator()( uint32_t a, uint32_t b ) const { return a > b ? a : b; }
};

int gridFor( uint64_t n )
{
	uint64_t b = ( n + BB - 1 ) / BB;
	if( b < 1 ) b = 1;
	return (int)( b > 4096 ? 4096 : b );
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
// The builder's device scalars, one zeroed 64-byte block: [0] fragment counter of the voxelizer, [8] hasEmission of the voxel set, [16] scalarOut (the total
// of scanCounts), [32] firstBad[2] and [48] edit counts[3] of the voxel-list calls
struct BuildScratch
{
	DevBuf b;
	unsigned long long* fragments() const { return b.as<unsigned long long>(); }
	uint32_t* hasEmission() const { return (uint32_t*)( fragments() + 1 ); }
	uint32_t* scalarOut() const { return (uint32_t*)( fragments() + 2 ); }
	unsigned long long* firstBad() const { return fragments() + 4; }
	uint32_t* counts() const { return (uint32_t*)( fragments() + 6 ); }
	int init( hipStream_t st )
	{
		if( b.alloc( 64 ) ) return 1;
		MVRT_HIP( hipMemsetAsync( b.p, 0, 64, st ) );
		return 0;
	}
	int initForLists( hipStream_t st ) // firstBad = none
	{
		if( init( st ) ) return 1;
		MVRT_HIP( hipMemsetAsync( firstBad(), 0xFF, 16, st ) );
		return 0;
	}
};

// second half of every stable compaction: the per-block counts a k...Count kernel left for nItems items become block offsets, their total goes to the host.
// Waits for the stream.
int scanCounts( const DevBuf& blockCnt, uint64_t nItems, const BuildScratch& sc, hipStream_t st, uint32_t* total )
{
	hipLaunchKernelGGL( kScanCounts, dim3( 1 ), dim3( 1024 ), 0, st, blockCnt.as<uint32_t>(), nItems, sc.scalarOut() );
	*total = 0;
	MVRT_HIP( hipMemcpyAsync( total, sc.scalarOut(), 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	return 0;
}

// (keysA, valsA): totalDumped unsorted fragments (released here) -> morton / attrs: the sorted unique codes and their integer-mean attributes; *hasEmission |= any emission
int sortUnique( DevBuf& keysA, DevBuf& valsA, unsigned long long totalDumped, int levels, hipStream_t st, const BuildScratch& sc, DevBuf& morton, DevBuf& attrs,
				uint32_t* nVoxelsOut )
{
	DevBuf keysB, valsB;
	if( keysB.alloc( totalDumped * 8 ) || valsB.alloc( totalDumped * 8 ) ) return 1;
	// ---- sort (IntersectorOctreeGPU.hpp:117-124) ----
	if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
			return hipcub::DeviceRadixSort::SortPairs( tmp, tmpBytes, keysA.as<uint64_t>(), keysB.as<uint64_t>(), valsA.as<uint64_t>(), valsB.as<uint64_t>(), (uint64_t)totalDumped, 0,
													   3 * levels, st );
		} ) )
		return 1;
	keysA.release();
	valsA.release();

	// ---- unique with integer-mean attributes (IntersectorOctreeGPU.hpp:126-137) ----
	DevBuf blockCnt;
	if( blockCnt.alloc( ( totalDumped / BB + 2 ) * 4 ) ) return 1;
	hipLaunchKernelGGL( kUniqueCount, dim3( gridFor( totalDumped ) ), dim3( BB ), 0, st, keysB.as<uint64_t>(), (uint64_t)totalDumped, blockCnt.as<uint32_t>() );
	uint32_t nVoxels = 0;
	if( scanCounts( blockCnt, totalDumped, sc, st, &nVoxels ) ) return 1;
	if( morton.alloc( (uint64_t)nVoxels * 8 ) || attrs.alloc( (uint64_t)nVoxels * 8 ) ) return 1;
	hipLaunchKernelGGL( kUniqueEmit, dim3( gridFor( totalDumped ) ), dim3( BB ), 0, st, keysB.as<uint64_t>(), valsB.as<uint64_t>(), (uint64_t)totalDumped,
						blockCnt.as<uint32_t>(), morton.as<uint64_t>(), attrs.as<uint2>(), sc.hasEmission() );
	MVRT_HIP( hipStreamSynchronize( st ) );
	*nVoxelsOut = nVoxels;
	return 0;
}

// The levels of one build, bottom-up.  A level turns the nInput tasks of `cur` (one per voxel, then one per node of the level below, in Morton order) into one
// task per sibling group in `nxt`, and the groups into nodes: a DAG level de-duplicates them, a direct or tree level (no DAG) writes every group to its final slot.
struct LevelBuild
{
	hipStream_t st;
	const BuildScratch& sc;
	int levels, flags;
	SvoBuildResult b; // filled as the levels go and handed over whole at the end: a failure on the way hands nothing over
	DevBuf blockCnt, tasksA, tasksB;
	Task *cur = nullptr, *nxt = nullptr;
	uint32_t nInput = 0, nGroups = 0, nodeBase = 0;
	std::vector<DevBuf> levelNodes, levelMasks; // DAG: the nodes of each level (levelMasks[l].bytes of them), concatenated at the end
	uint32_t treeBrickBase[24] = { 0 };			// tree: first brick of each (odd) builder level

	int start( const DevBuf& morton, uint32_t nVoxels )
	{
		if( blockCnt.alloc( ( (uint64_t)nVoxels / BB + 2 ) * 4 ) ) return 1;
		if( tasksA.alloc( (uint64_t)nVoxels * sizeof( Task ) ) || tasksB.alloc( (uint64_t)nVoxels * sizeof( Task ) ) ) return 1;
		hipLaunchKernelGGL( kInitTasks, dim3( gridFor( nVoxels ) ), dim3( BB ), 0, st, morton.as<uint64_t>(), nVoxels, tasksA.as<Task>() );
		cur = tasksA.as<Task>();
		nxt = tasksB.as<Task>();
		nInput = nVoxels;
		return 0;
	}
	// sibling groups of `cur`: nGroups, and in blockCnt the offsets every level kernel ranks its group heads with
	int countGroups()
	{
		hipLaunchKernelGGL( kGroupCount, dim3( gridFor( nInput ) ), dim3( BB ), 0, st, cur, (uint64_t)nInput, blockCnt.as<uint32_t>() );
		return scanCounts( blockCnt, nInput, sc, st, &nGroups );
	}

	// ---- DAG: a candidate node per group; equal-content candidates collapse onto their first group; the first occurrences become this level's nodes, numbered
	// in group order (the creation order of the CPU reference).  *nUnique of them.  The scratch of the level is released on return.
	int dagLevel( uint32_t* nUnique )
	{
		const uint64_t n = nGroups;
		DevBuf cands, hashes, groupIds, parents, hashesS, groupS, headPos, headScan, repOf, nodeOfGroup, blockCnt2;
		if( cands.alloc( n * sizeof( Cand ) ) || hashes.alloc( n * 8 ) || groupIds.alloc( n * 4 ) || parents.alloc( n * 8 ) || hashesS.alloc( n * 8 ) || groupS.alloc( n * 4 ) ||
			headPos.alloc( n * 4 ) || headScan.alloc( n * 4 ) || repOf.alloc( n * 4 ) || nodeOfGroup.alloc( n * 4 ) || blockCnt2.alloc( ( n / BB + 2 ) * 4 ) )
			return 1;
		const dim3 grid( gridFor( nGroups ) ), block( BB );
		hipLaunchKernelGGL( kMakeCandidates, dim3( gridFor( nInput ) ), block, 0, st, cur, (uint64_t)nInput, blockCnt.as<uint32_t>(), cands.as<Cand>(), hashes.as<uint64_t>(),
							groupIds.as<uint32_t>(), parents.as<uint64_t>() );
		// de-duplication by sorted content hash: repOf[group] = the first group with its content.  Not two withCubTemp calls: each would allocate and wait for the
		// stream; here the sort and the scan share one temporary of the larger size and the five steps are enqueued back to back, with one wait at the end
		{
			const auto sort = [&]( void* tmp, size_t& bytes ) {
				return hipcub::DeviceRadixSort::SortPairs( tmp, bytes, hashes.as<uint64_t>(), hashesS.as<uint64_t>(), groupIds.as<uint32_t>(), groupS.as<uint32_t>(), nGroups, 0, 64, st );
			};
			const auto scan = [&]( void* tmp, size_t& bytes ) {
				return hipcub::DeviceScan::InclusiveScan( tmp, bytes, headPos.as<uint32_t>(), headScan.as<uint32_t>(), MaxOp(), nGroups, st );
			};
			size_t sortBytes = 0, scanBytes = 0;
			MVRT_HIP( sort( nullptr, sortBytes ) );
			MVRT_HIP( scan( nullptr, scanBytes ) );
			DevBuf tmp;
			if( tmp.alloc( sortBytes > scanBytes ? sortBytes : scanBytes ) ) return 1;
			MVRT_HIP( sort( tmp.p, sortBytes ) );
			hipLaunchKernelGGL( kMarkRuns, grid, block, 0, st, hashesS.as<uint64_t>(), groupS.as<uint32_t>(), cands.as<Cand>(), nGroups, headPos.as<uint32_t>() );
			MVRT_HIP( scan( tmp.p, scanBytes ) );
			hipLaunchKernelGGL( kScatterReps, grid, block, 0, st, groupS.as<uint32_t>(), headScan.as<uint32_t>(), nGroups, repOf.as<uint32_t>() );
			MVRT_HIP( hipStreamSynchronize( st ) ); // tmp is released at scope end
		}
		// number the first occurrences in group order and write their nodes
		hipLaunchKernelGGL( kFirstCount, grid, block, 0, st, repOf.as<uint32_t>(), n, blockCnt2.as<uint32_t>() );
		if( scanCounts( blockCnt2, n, sc, st, nUnique ) ) return 1;
		levelNodes.emplace_back();
		levelMasks.emplace_back();
		if( levelNodes.back().alloc( (uint64_t)*nUnique * sizeof( Node64 ) ) || levelMasks.back().alloc( *nUnique ) ) return 1;
		// kEmitNodes writes to nodes[nodeBase + rank]: pass pointers rebased so that index nodeBase lands on the level's first node
		hipLaunchKernelGGL( kEmitNodes, grid, block, 0, st, repOf.as<uint32_t>(), cands.as<Cand>(), n, blockCnt2.as<uint32_t>(), nodeBase, levelNodes.back().as<Node64>() - nodeBase,
							levelMasks.back().as<uint8_t>() - nodeBase, nodeOfGroup.as<uint32_t>() );
		hipLaunchKernelGGL( kNextTasks, grid, block, 0, st, repOf.as<uint32_t>(), nodeOfGroup.as<uint32_t>(), cands.as<Cand>(), parents.as<uint64_t>(), nGroups, nxt );
		MVRT_HIP( hipStreamSynchronize( st ) );
		return 0;
	}
	// the per-level arrays -> b.nodes / b.masks
	int concatLevels()
	{
		if( b.nodes.alloc( (uint64_t)nodeBase * sizeof( Node64 ) ) || b.masks.alloc( nodeBase ) ) return 1;
		uint64_t off = 0;
		for( size_t l = 0; l < levelNodes.size(); l++ )
		{
			const uint64_t count = levelMasks[l].bytes;
			MVRT_HIP( hipMemcpyAsync( b.nodes.as<Node64>() + off, levelNodes[l].p, count * sizeof( Node64 ), hipMemcpyDeviceToDevice, st ) );
			MVRT_HIP( hipMemcpyAsync( b.masks.as<uint8_t>() + off, levelMasks[l].p, count, hipMemcpyDeviceToDevice, st ) );
			off += count;
		}
		MVRT_HIP( hipStreamSynchronize( st ) );
		levelNodes.clear();
		levelMasks.clear();
		return 0;
	}

	// ---- no DAG: every group is a node.  Before the first level: distinct parents per level in one pass (octreeTaskInit's taskCounters, voxKernel.cu:257-265) ->
	// exact node count -> the final arrays in one allocation each, and which of the two flavours fills them
	int sizeNoDag( const DevBuf& morton, uint32_t nVoxels )
	{
		DevBuf dCounts;
		if( dCounts.alloc( 32 * 8 ) ) return 1;
		MVRT_HIP( hipMemsetAsync( dCounts.p, 0, 32 * 8, st ) );
		hipLaunchKernelGGL( kLevelCounts, dim3( gridFor( nVoxels ) ), dim3( BB ), 0, st, morton.as<uint64_t>(), (uint64_t)nVoxels, levels, dCounts.as<unsigned long long>() );
		unsigned long long hc[32];
		MVRT_HIP( hipMemcpyAsync( hc, dCounts.p, sizeof( hc ), hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
		unsigned long long total = 0;
		for( int l = 0; l < levels; l++ ) total += hc[l];
		if( total >= 0xFFFFFFFEull )
		{
			mvrtSetError( "mvrt_svo_build: %llu nodes exceed 32-bit node indices", total );
			return 1;
		}
		// no embedded masks (too many nodes, or switched off): compact { mask, first child } nodes + two-level bricks instead of 64-byte lines per node
		b.tree = total >= 0xFFFFFFull || ( flags & 2 );
		if( b.masks.alloc( total ) ) return 1;
		if( !b.tree ) return b.nodes.alloc( total * sizeof( Node64 ) );
		// node ranges per builder level (0 = parents of voxels ... levels - 1 = root) and brick ranges of the odd levels
		unsigned long long nb = 0, nBr = 0;
		for( int l = 0; l < levels; l++ )
		{
			b.treeLevelBase[l] = (uint32_t)nb;
			b.treeLevelCount[l] = (uint32_t)hc[l];
			treeBrickBase[l] = (uint32_t)nBr;
			nb += hc[l];
			if( l & 1 ) nBr += hc[l];
		}
		b.nBricks = (uint32_t)nBr;
		// where the traversal starts: the root is the single node of builder level levels - 1.  Odd level: it is a brick root -> its brick.
		// Even level: it is an "in-brick child" whose children (level levels - 2) are brick roots -> the first of them (or, for a one-level
		// octree, voxel 0)
		const int rl = levels - 1;
		b.treeRoot = ( rl & 1 ) ? treeBrickBase[rl] : ( rl == 0 ? 0u : treeBrickBase[rl - 1] );
		return b.treeFirst.alloc( total * 4 ) || b.nodes.alloc( ( nBr ? nBr : 1 ) * sizeof( uint4 ) );
	}
	int directLevel()
	{
		hipLaunchKernelGGL( kMakeNodesDirect, dim3( gridFor( nInput ) ), dim3( BB ), 0, st, cur, (uint64_t)nInput, blockCnt.as<uint32_t>(), nodeBase, b.nodes.as<Node64>(),
							b.masks.as<uint8_t>(), nxt );
		MVRT_HIP( hipStreamSynchronize( st ) );
		return 0;
	}
	int treeLevel( int level ) // its nodes, and for an odd level their bricks (b.nodes)
	{
		hipLaunchKernelGGL( kMakeNodesTree, dim3( gridFor( nInput ) ), dim3( BB ), 0, st, cur, (uint64_t)nInput, blockCnt.as<uint32_t>(), nodeBase, level == 0 ? 1 : 0,
							b.masks.as<uint8_t>(), b.treeFirst.as<uint32_t>(), nxt );
		if( level & 1 )
			hipLaunchKernelGGL( kMakeBricks, dim3( gridFor( nGroups ) ), dim3( BB ), 0, st, b.masks.as<uint8_t>(), b.treeFirst.as<uint32_t>(), b.treeLevelBase[level], nGroups,
								level - 1 == 0 ? 1 : 0, level >= 2 ? b.treeLevelBase[level - 2] : 0u, level >= 2 ? treeBrickBase[level - 2] : 0u,
								b.nodes.as<uint4>() + treeBrickBase[level] );
		MVRT_HIP( hipStreamSynchronize( st ) );
		return 0;
	}

	// ---- 64-byte nodes, DAG or direct: child masks into the child pointers (embedded flavour), or nVoxelsPSum -> cold array and child masks -> the hot line
	// (plain flavour, traverse_stream.h).  The tree flavour has nothing left to convert: the traversal reads the bricks, download rebuilds the reference's nodes
	int finishNodes()
	{
		const uint32_t nNodes = nodeBase;
		b.embedded = nNodes < 0xFFFFFFu && !( flags & 2 ) ? 1 : 0;
		if( b.embedded )
		{
			hipLaunchKernelGGL( kEmbedMasks, dim3( divUp( (uint64_t)nNodes * 8, BB ) ), dim3( BB ), 0, st, b.nodes.as<Node64>(), b.masks.as<uint8_t>(), nNodes );
			return 0;
		}
		if( b.psumCold.alloc( (uint64_t)nNodes * 32 ) ) return 1;
		return launchSplitPsum( b.nodes.as<Node64>(), b.masks.as<uint8_t>(), b.psumCold.as<uint32_t>(), nNodes, st );
	}
};

// the levels of the octree over nVoxels sorted unique codes (morton / attrs are handed to *out on success); sc.hasEmission(): the device flag of the voxel set
int buildLevels( DevBuf& morton, DevBuf& attrs, uint32_t nVoxels, unsigned long long totalDumped, int gridRes, int flags, hipStream_t st, const BuildScratch& sc,
				 SvoBuildResult* out )
{
	const bool dag = !( flags & 1 );
	LevelBuild lb{ st, sc, levelsOf( gridRes ), flags };
	if( lb.start( morton, nVoxels ) ) return 1;
	for( int level = 0; level < lb.levels; level++ )
	{
		if( lb.countGroups() ) return 1;
		uint32_t nNew = lb.nGroups; // nodes of this level
		if( dag )
		{
			if( lb.dagLevel( &nNew ) ) return 1;
		}
		else
		{
			if( level == 0 && lb.sizeNoDag( morton, nVoxels ) ) return 1;
			if( lb.b.tree ? lb.treeLevel( level ) : lb.directLevel() ) return 1;
		}
		lb.nodeBase += nNew;
		lb.nInput = lb.nGroups;
		std::swap( lb.cur, lb.nxt );
	}
	if( lb.nInput != 1 )
	{
		mvrtSetError( "mvrt_svo_build: internal error, %u roots after %d levels", lb.nInput, lb.levels );
		return 1;
	}
	if( dag && lb.concatLevels() ) return 1;
	if( !lb.b.tree && lb.finishNodes() ) return 1;
	SvoBuildResult& b = lb.b;
	MVRT_HIP( hipMemcpyAsync( &b.hasEmission, sc.hasEmission(), 4, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	MVRT_HIP( hipGetLastError() );
	b.attrs = std::move( attrs );
	b.morton = std::move( morton );
	b.nNodes = lb.nodeBase;
	b.nVoxels = nVoxels;
	b.totalDumped = totalDumped;
	*out = std::move( b );
	return 0;
}

// everything after voxelization: sort + unique of the (Morton, attribute) fragments, then the levels
int buildFromFragments( DevBuf& keysA, DevBuf& valsA, unsigned long long totalDumped, int gridRes, int flags, hipStream_t st, const BuildScratch& sc, SvoBuildResult* out )
{
	DevBuf morton, attrs;
	uint32_t nVoxels = 0;
	if( sortUnique( keysA, valsA, totalDumped, levelsOf( gridRes ), st, sc, morton, attrs, &nVoxels ) ) return 1;
	return buildLevels( morton, attrs, nVoxels, totalDumped, gridRes, flags, st, sc, out );
}

} // namespace

int svoBuildFromTriangles( const float* vertsHost, const float* colsHost, const float* emisHost, uint64_t nVertices, f3 origin, float dps, int gridRes, int flags, hipStream_t st,
						   SvoBuildResult* out )
{
	const uint32_t nTri = (uint32_t)( nVertices / 3 );

	DevBuf dVerts, dCols, dEmis;
	BuildScratch sc;
	if( dVerts.alloc( nVertices * 12 ) || sc.init( st ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( dVerts.p, vertsHost, nVertices * 12, hipMemcpyHostToDevice, st ) );
	if( colsHost )
	{
		if( dCols.alloc( nVertices * 12 ) ) return 1;
		MVRT_HIP( hipMemcpyAsync( dCols.p, colsHost, nVertices * 12, hipMemcpyHostToDevice, st ) );
	}
	if( emisHost )
	{
		if( dEmis.alloc( nVertices * 12 ) ) return 1;
		MVRT_HIP( hipMemcpyAsync( dEmis.p, emisHost, nVertices * 12, hipMemcpyHostToDevice, st ) );
	}

	// ---- voxelize: count, allocate, emit (IntersectorOctreeGPU.hpp:81-116) ----
	const uint32_t triGrid = divUp( nTri, 128 );
	hipLaunchKernelGGL( kVoxelize<false>, dim3( triGrid ), dim3( 128 ), 0, st, dVerts.as<float>(), (const float*)nullptr, (const float*)nullptr, nTri, sc.fragments(), origin, dps,
						gridRes, (uint64_t*)nullptr, (uint64_t*)nullptr, ( flags & 4 ) ? 1 : 0 );
	unsigned long long totalDumped = 0;
	MVRT_HIP( hipMemcpyAsync( &totalDumped, sc.fragments(), 8, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	if( totalDumped == 0 )
	{
		mvrtSetError( "mvrt_svo_build: the triangles touch no voxel of the grid" );
		return 1;
	}
	if( totalDumped >= 0xFFFFFFFFull )
	{
		mvrtSetError( "mvrt_svo_build: %llu voxel fragments exceed the 32-bit index range of this builder", totalDumped );
		return 1;
	}
	DevBuf keysA, valsA;
	if( keysA.alloc( totalDumped * 8 ) || valsA.alloc( totalDumped * 8 ) ) return 1;
	MVRT_HIP( hipMemsetAsync( sc.fragments(), 0, 8, st ) );
	hipLaunchKernelGGL( kVoxelize<true>, dim3( triGrid ), dim3( 128 ), 0, st, dVerts.as<float>(), dCols.as<float>(), dEmis.as<float>(), nTri, sc.fragments(), origin, dps, gridRes,
						keysA.as<uint64_t>(), valsA.as<uint64_t>(), ( flags & 4 ) ? 1 : 0 );

	dVerts.release();
	dCols.release();
	dEmis.release();
	return buildFromFragments( keysA, valsA, totalDumped, gridRes, flags, st, sc, out );
}

int svoBuildSynthetic( uint64_t nRandomVoxels, uint64_t seed, int gridRes, int flags, hipStream_t st, SvoBuildResult* out )
{
	if( nRandomVoxels == 0 || nRandomVoxels >= 0xFFFFFFFFull )
	{
		mvrtSetError( "mvrt_svo_build_synthetic: voxel count must be in [1, 2^32-2]" );
		return 1;
	}
	BuildScratch sc;
	DevBuf keysA, valsA;
	if( sc.init( st ) || keysA.alloc( nRandomVoxels * 8 ) || valsA.alloc( nRandomVoxels * 8 ) ) return 1;
	hipLaunchKernelGGL( kSyntheticVoxels, dim3( gridFor( nRandomVoxels ) ), dim3( BB ), 0, st, nRandomVoxels, seed, (uint32_t)gridRes, keysA.as<uint64_t>(), valsA.as<uint64_t>() );
	return buildFromFragments( keysA, valsA, nRandomVoxels, gridRes, flags, st, sc, out );
}

// ---- voxel lists ----------------------------------------------------------------------------------------------------------------------------
// encode + validate n entries into keys / vals (/ idx); a failure names the lowest offending entry
static int encodeVoxels( const char* who, const uint32_t* xyz, const uint32_t* attribs, const uint8_t* ops, uint64_t n, int gridRes, hipStream_t st, const BuildScratch& sc,
						 uint64_t* keys, uint64_t* vals, uint32_t* idx )
{
	const int vec = ( (uintptr_t)xyz % 16 == 0 && (uintptr_t)attribs % 16 == 0 ) ? 1 : 0;
	hipLaunchKernelGGL( kEncodeVoxels, dim3( gridFor( ( n + ENC_PER - 1 ) / ENC_PER ) ), dim3( BB ), 0, st, xyz, attribs, ops, n, (uint32_t)gridRes, vec, keys, vals, idx,
						sc.firstBad() );
	unsigned long long bad[2] = { 0, 0 };
	MVRT_HIP( hipMemcpyAsync( bad, sc.firstBad(), 16, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	if( bad[0] != ~0ull )
	{
		uint32_t c[3] = { 0, 0, 0 };
		MVRT_HIP( hipMemcpy( c, xyz + bad[0] * 3, 12, hipMemcpyDeviceToHost ) ); // (default stream: the caller's array, behind the hipStreamSynchronize( st ) above)
		mvrtSetError( "%s: entry %llu (%u, %u, %u) lies outside the %d^3 grid", who, bad[0], c[0], c[1], c[2], gridRes );
		return 1;
	}
	if( bad[1] != ~0ull )
	{
		uint8_t op = 0;
		MVRT_HIP( hipMemcpy( &op, ops + bad[1], 1, hipMemcpyDeviceToHost ) ); // (default stream: the caller's array, behind the hipStreamSynchronize( st ) above)
		mvrtSetError( "%s: entry %llu has the unknown op %u (MVRT_VOXEL_REMOVE = 0, MVRT_VOXEL_SET = 1)", who, bad[1], (unsigned)op );
		return 1;
	}
	return 0;
}

int svoBuildFromVoxels( const uint32_t* xyz, const uint32_t* attribs, uint64_t n, int gridRes, int flags, hipStream_t st, SvoBuildResult* out )
{
	BuildScratch sc;
	DevBuf keysA, valsA;
	if( sc.initForLists( st ) || keysA.alloc( n * 8 ) || valsA.alloc( n * 8 ) ) return 1;
	if( encodeVoxels( "mvrt_svo_build_voxels", xyz, attribs, nullptr, n, gridRes, st, sc, keysA.as<uint64_t>(), valsA.as<uint64_t>(), nullptr ) ) return 1;
	return buildFromFragments( keysA, valsA, n, gridRes, flags, st, sc, out );
}

int svoBuildFromSorted( DevBuf& morton, DevBuf& attrs, uint32_t n, int gridRes, int flags, hipStream_t st, SvoBuildResult* out )
{
	BuildScratch sc;
	if( sc.initForLists( st ) ) return 1;
	return buildLevels( morton, attrs, n, n, gridRes, flags, st, sc, out );
}

int svoEditVoxels( const uint64_t* oldMorton, uint2* oldAttrs, uint32_t nOld, const uint32_t* xyz, const uint32_t* attribs, const uint8_t* ops, uint64_t n, int gridRes, int flags,
				   hipStream_t st, SvoBuildResult* out, int* structural, uint32_t* hasEmissionOut )
{
	static const char* who = "mvrt_svo_edit_voxels";
	const int levels = levelsOf( gridRes );
	BuildScratch sc;
	DevBuf keysA, attrN, idxA, keysB, idxB;
	if( sc.initForLists( st ) || keysA.alloc( n * 8 ) || attrN.alloc( n * 8 ) || idxA.alloc( n * 4 ) || keysB.alloc( n * 8 ) || idxB.alloc( n * 4 ) ) return 1;
	if( encodeVoxels( who, xyz, attribs, ops, n, gridRes, st, sc, keysA.as<uint64_t>(), attrN.as<uint64_t>(), idxA.as<uint32_t>() ) ) return 1;
	// stable sort of (Morton, batch index): within a key the batch order survives, its last entry wins
	if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
			return hipcub::DeviceRadixSort::SortPairs( tmp, tmpBytes, keysA.as<uint64_t>(), keysB.as<uint64_t>(), idxA.as<uint32_t>(), idxB.as<uint32_t>(), n, 0, 3 * levels, st );
		} ) )
		return 1;
	keysA.release();
	idxA.release();
	// last entry per key -> the sorted unique edit list, classified against the old list
	DevBuf blockCnt;
	if( blockCnt.alloc( ( n / BB + 2 ) * 4 ) ) return 1;
	hipLaunchKernelGGL( kEditTailCount, dim3( gridFor( n ) ), dim3( BB ), 0, st, keysB.as<uint64_t>(), n, blockCnt.as<uint32_t>() );
	uint32_t nE = 0;
	if( scanCounts( blockCnt, n, sc, st, &nE ) ) return 1;
	DevBuf eKeys, eAttr, ePos, eKind, eInc, ePre;
	if( eKeys.alloc( (uint64_t)nE * 8 ) || eAttr.alloc( (uint64_t)nE * 8 ) || ePos.alloc( (uint64_t)nE * 4 ) || eKind.alloc( nE ) || eInc.alloc( ( (uint64_t)nE + 1 ) * 8 ) ||
		ePre.alloc( ( (uint64_t)nE + 1 ) * 8 ) )
		return 1;
	MVRT_HIP( hipMemsetAsync( eInc.as<uint64_t>() + nE, 0, 8, st ) );
	hipLaunchKernelGGL( kEditClassify, dim3( gridFor( n ) ), dim3( BB ), 0, st, keysB.as<uint64_t>(), idxB.as<uint32_t>(), n, blockCnt.as<uint32_t>(), attrN.as<uint64_t>(), ops,
						oldMorton, nOld, eKeys.as<uint64_t>(), eAttr.as<uint64_t>(), ePos.as<uint32_t>(), eKind.as<uint8_t>(), eInc.as<unsigned long long>(), sc.counts() );
	uint32_t counts[3] = { 0, 0, 0 };
	MVRT_HIP( hipMemcpyAsync( counts, sc.counts(), 12, hipMemcpyDeviceToHost, st ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	keysB.release();
	idxB.release();
	attrN.release();
	const uint32_t nIns = counts[0], nRem = counts[1];
	if( nIns == 0 && nRem == 0 ) // attribute-only (or nothing to do): the node structure stays, attributes change in place
	{
		if( nE ) hipLaunchKernelGGL( kScatterAttrs, dim3( gridFor( nE ) ), dim3( BB ), 0, st, eAttr.as<uint64_t>(), eKind.as<uint8_t>(), ePos.as<uint32_t>(), nE, oldAttrs );
		hipLaunchKernelGGL( kAnyEmission, dim3( gridFor( ( (uint64_t)nOld + 1 ) / 2 ) ), dim3( BB ), 0, st, (const uint2*)oldAttrs, nOld, sc.hasEmission() );
		uint32_t he = 0;
		MVRT_HIP( hipMemcpyAsync( &he, sc.hasEmission(), 4, hipMemcpyDeviceToHost, st ) );
		MVRT_HIP( hipStreamSynchronize( st ) );
		MVRT_HIP( hipGetLastError() );
		*structural = 0;
		*hasEmissionOut = he;
		return 0;
	}
	if( (uint64_t)nOld + nIns - nRem == 0 )
	{
		mvrtSetError( "%s: the edit would remove every voxel of the octree", who );
		return 1;
	}
	if( (uint64_t)nOld + nIns >= 0xFFFFFFFFull )
	{
		mvrtSetError( "%s: %llu voxels exceed the 32-bit index range of this builder", who, (unsigned long long)nOld + nIns );
		return 1;
	}
	const uint32_t nNew = nOld + nIns - nRem;
	if( withCubTemp( st, [&]( void* tmp, size_t& tmpBytes ) {
			return hipcub::DeviceScan::ExclusiveSum( tmp, tmpBytes, eInc.as<unsigned long long>(), ePre.as<unsigned long long>(), nE + 1, st );
		} ) )
		return 1;
	DevBuf morton, attrs;
	if( morton.alloc( (uint64_t)nNew * 8 ) || attrs.alloc( (uint64_t)nNew * 8 ) ) return 1;
	hipLaunchKernelGGL( kMergeOld, dim3( gridFor( ( (uint64_t)nOld + MERGE_PER - 1 ) / MERGE_PER ) ), dim3( BB ), 0, st, oldMorton, (const uint2*)oldAttrs, nOld, eKeys.as<uint64_t>(),
						eAttr.as<uint64_t>(), eKind.as<uint8_t>(), ePre.as<unsigned long long>(), nE, morton.as<uint64_t>(), attrs.as<uint2>(), sc.hasEmission() );
	hipLaunchKernelGGL( kMergeInserts, dim3( gridFor( nE ) ), dim3( BB ), 0, st, eKeys.as<uint64_t>(), eAttr.as<uint64_t>(), eKind.as<uint8_t>(), ePos.as<uint32_t>(),
						ePre.as<unsigned long long>(), nE, morton.as<uint64_t>(), attrs.as<uint2>(), sc.hasEmission() );
	MVRT_HIP( hipStreamSynchronize( st ) );
	eKeys.release();
	eAttr.release();
	ePos.release();
	eKind.release();
	eInc.release();
	ePre.release();
	*structural = 1;
	return buildLevels( morton, attrs, nNew, 0, gridRes, flags, st, sc, out );
}
