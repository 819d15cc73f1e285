// device.hpp -- per-thread octree traversal for application HIP kernels (header-only, gfx950).
//
// The reference's user kernels take IntersectorOctreeGPU BY VALUE and call its device methods per thread
// (IntersectorOctreeGPU.hpp:243-264; voxKernel.cu:437-483 `render` is one).  mvrt::DeviceOctree is that struct for octrees
// owned by libmvrt_hip.so: fill an mvrt_device_octree with mvrt_svo_device_view() (include/mvrt.h) on the host, pass it to
// your kernel by value, wrap it in a DeviceOctree and call
//
//     intersect( ro, rd, &t, &nMajor, &vIndex, isShadowRay )            stack kept by the thread (scratch memory)
//     intersect( stack, ro, rd, &t, &nMajor, &vIndex, isShadowRay )     caller's stack: levels entries of 16 bytes, LDS or global
//     intersectEx( ..., &descents )                                     + child fetches per ray (voxCommon.hpp:381)
//     intersectRange( [stack,] ro, rd, tMax, &t, &nMajor, &vIndex, isShadowRay )   the same ray, limited to t <= tMax (see below)
//     intersectRangeEx( ..., &descents )
//     occluded( [stack,] ro, rd, tMax )                                 shadow ray with the limit: true when something is hit within tMax
//     intersectCone( [stack,] ro, rd, coneA, coneB, &t, &nMajor, &level, &cellCode )   the same ray, stopped at its own level of detail (see below)
//     intersectConeEx( ..., &descents )
//     getVoxelColor( vIndex ), getVoxelEmission( vIndex, withScale ), hasEmission()
//
// Results equal mvrt_trace_batch's bit for bit (t, nMajor, vIndex, descents; MVRT_MAX_FLOAT / -1 / 0 on a miss, vIndex 0 for
// shadow rays), for both octree flavours the view accepts (MVRT_FLAVOUR_EMBEDDED, MVRT_FLAVOUR_PLAIN).  The walk is the
// reference's octreeTraverse_EfficientParametric (voxCommon.hpp:231-423) one candidate child at a time, with the library's
// 16-byte stack entries in level-indexed slots (traverse_stream.h): the pending levels are a 32-bit mask (pop = highest set
// bit), the candidate a popped node resumes with rides in a 3-bits-per-level register, the hit voxel's path in another.  vIndex
// is the sum of the stored nVoxelsPSum along that path, read after the hit.
//
// Distance limit: a ray with limit tMax reports what the unlimited ray reports when that ray hits with t <= tMax (t in units of rd), and a miss
// otherwise -- bit for bit, for every ray, so a NaN tMax or one that is not above 0 always misses, +inf changes nothing, and MVRT_MAX_FLOAT changes nothing
// but this: a ray without a direction (every component zero or denormal) can "hit" at t = +inf as in the reference, and inf <= MVRT_MAX_FLOAT is
// false, so under MVRT_MAX_FLOAT that ray misses and under +inf it hits (occluded() likewise).  The walk
// stops early once the candidate child's entry time exceeds tMax by a margin that covers the fp32 rounding of the entry times along the walk
// (DESIGN.md 5.12 derives it); rays whose slab deltas are not all finite are never cut, only filtered.  descents of a limited ray = the child
// fetches it made: at most the unlimited ray's, equal to them on an accepted hit.
//
// Cone limit: the ray's footprint at time S is f = coneA + coneB * S (one product, one sum, each rounded).  On the FIRST visit of an inner node
// at level in [1, levels - 1], with S = the node's entry time of that iteration, the node is terminal iff 0 < S and size <= f, size = dps * 2^levels * 2^-level
// (exact).  A terminal node reports the hit a voxel in its place would: t = S, nMajor by the voxel's rule, level = the node's level, cellCode = the path to it (3
// bits per level = the Morton code of any voxel below it >> 3 * ( levels - level )).  A voxel hit reports level = levels and the voxel's Morton code; a miss
// MVRT_MAX_FLOAT, -1, 0, 0.  The root is never terminal, a node with S <= 0 is descended into as always, and a node is not tested again after a pop.  Every slab
// time derives from the root's times and the level alone, so a walk stopped at depth D reports bit for bit the t and nMajor of the same ray against the octree
// coarsened to D levels (mvrt_svo_coarsen keeps lower and upper bit-identical).  What follows from the rule:
//   * coneA = coneB = 0, any negative footprint and NaN give the unlimited ray's t, nMajor and descents, bit for bit (the compare is false for them);
//   * the cone ray's descents never exceed the unlimited ray's: it is the same walk up to the first terminal node;
//   * where the unlimited ray hits, the cone ray hits too (at that voxel or at a node on the walk before it);
//   * a cone ray may hit where the unlimited ray misses: a coarse cell is solid to it.
//
// Floating point: bit-exactness needs every product and sum rounded on its own.  Every function here that does fp32 arithmetic
// opens with `#pragma clang fp contract(off)`, which clang honours under hipcc's default and under -ffp-contract=on.
//   * -ffast-math is refused below (#error).
//   * -ffp-contract=fast is NOT SUPPORTED: it overrides the pragma (a*b+c becomes v_fma) and no macro reveals it, so this
//     header cannot detect it.  Results then differ from mvrt_trace_batch in the last bits of t and in tie-breaks.
#pragma once
#if defined( __FAST_MATH__ )
#error "mvrt/device.hpp: -ffast-math is not supported: the octree traversal is bit-exact only with IEEE fp32 arithmetic (also avoid -ffp-contract=fast)"
#endif

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mvrt.h"

#define MVRT_DEVICE_FP_STRICT _Pragma( "clang fp contract(off)" )

namespace mvrt
{
// one saved node: its reference (index, embedded flavour: | own mask << 24) and its exit times
struct alignas( 16 ) StackEntry
{
	uint32_t node;
	float tx1, ty1, tz1;
};
static_assert( sizeof( StackEntry ) == 16, "StackEntry is 16 bytes" );

namespace detail
{
constexpr float kMaxFloat = 3.402823466e+38F; // reference MAX_FLOAT, vectorMath.hpp:79
constexpr uint32_t kLeaf = 0xFFFFFFFFu;		  // child pointer of a voxel, voxKernel.cu:254,299
// the reference's ss_max / ss_min are plain ternaries (vectorMath.hpp:100-108): keep their argument order
__host__ __device__ inline float smax( float x, float y ) { return ( x < y ) ? y : x; }
__host__ __device__ inline float smin( float x, float y ) { return ( y < x ) ? y : x; }
__host__ __device__ inline float sabs( float x ) { return x >= 0.0f ? x : -x; }
__host__ __device__ inline float max3( float a, float b, float c ) { return smax( smax( a, b ), c ); }
__host__ __device__ inline float min3( float a, float b, float c ) { return smin( smin( a, b ), c ); }
__host__ __device__ inline float mix( float a, float b, float t )
{
	MVRT_DEVICE_FP_STRICT
	return a + ( b - a ) * t;
}
struct Line64 // a node line: children[8], then nVoxelsPSum[8] (embedded) or the 8 child masks in psum[0..1] (plain)
{
	uint32_t children[8];
	uint32_t psum[8];
};
} // namespace detail

// normal of the face hit along major axis nMajor (voxCommon.hpp:564-577)
__host__ __device__ inline float3 getHitN( int major, float3 rd )
{
	float3 n = make_float3( 0.0f, 0.0f, 0.0f );
	if( major == 0 ) n.z = 0.0f < rd.z ? -1.0f : 1.0f;
	else if( major == 1 ) n.x = 0.0f < rd.x ? -1.0f : 1.0f;
	else if( major == 2 ) n.y = 0.0f < rd.y ? -1.0f : 1.0f;
	return n;
}

// the reference's CameraPinhole (renderCommon.hpp:17-84) on the 15-float camera of the C-ABI: {o, front, up, right, tanHthetaY, lensR, focus}
struct CameraPinhole
{
	float3 m_o, m_front, m_up, m_right;
	float m_tanHthetaY, m_lensR, m_focus;

	CameraPinhole() = default;
	__host__ __device__ explicit CameraPinhole( const float c[15] )
	{
		m_o = make_float3( c[0], c[1], c[2] );
		m_front = make_float3( c[3], c[4], c[5] );
		m_up = make_float3( c[6], c[7], c[8] );
		m_right = make_float3( c[9], c[10], c[11] );
		m_tanHthetaY = c[12];
		m_lensR = c[13];
		m_focus = c[14];
	}
	// :37-49 -- the operations of mvrt_render_primary's camera, in the same order
	__host__ __device__ void shoot( float3* ro, float3* rd, int x, int y, float xo, float yo, int W, int H ) const
	{
		MVRT_DEVICE_FP_STRICT
		const float xf = ( x + xo ) / W;
		const float yf = ( y + yo ) / H;
		const float a = detail::mix( -m_tanHthetaY, m_tanHthetaY, xf );
		const float b = detail::mix( m_tanHthetaY, -m_tanHthetaY, yf );
		const float w = (float)W, h = (float)H;
		*ro = m_o;
		*rd = make_float3( m_right.x * a * w / h + m_up.x * b + m_front.x, m_right.y * a * w / h + m_up.y * b + m_front.y, m_right.z * a * w / h + m_up.z * b + m_front.z );
	}
	// :50-75
	__host__ __device__ void shootThinLens( float3* ro, float3* rd, int x, int y, float xo, float yo, int W, int H, float u0, float u1 ) const
	{
		MVRT_DEVICE_FP_STRICT
		const float xf = ( x + xo ) / W;
		const float yf = ( y + yo ) / H;
		const float fx = m_focus * detail::mix( -m_tanHthetaY, m_tanHthetaY, xf ) * (float)W / (float)H;
		const float fy = m_focus * detail::mix( m_tanHthetaY, -m_tanHthetaY, yf );
		const float fz = m_focus;
		const float lx = detail::mix( -m_lensR, m_lensR, u0 ), ly = detail::mix( -m_lensR, m_lensR, u1 ), lz = 0.0f;
		const float dx = fx - lx, dy = fy - ly, dz = fz - lz;
		*rd = make_float3( m_right.x * dx + m_up.x * dy + m_front.x * dz, m_right.y * dx + m_up.y * dy + m_front.y * dz, m_right.z * dx + m_up.z * dy + m_front.z * dz );
		*ro = make_float3( m_o.x + m_right.x * lx + m_up.x * ly + m_front.x * lz, m_o.y + m_right.y * lx + m_up.y * ly + m_front.y * lz,
						   m_o.z + m_right.z * lx + m_up.z * ly + m_front.z * lz );
	}
};
static_assert( sizeof( CameraPinhole ) == 60, "CameraPinhole must match the reference's 60-byte layout" );

struct DeviceOctree
{
	mvrt_device_octree view;

	DeviceOctree() = default;
	__host__ __device__ explicit DeviceOctree( const mvrt_device_octree& v ) : view( v ) {}

	__host__ __device__ bool hasEmission() const { return view.hasEmission != 0; } // :261-264
	__device__ uchar4 getVoxelColor( uint32_t vIndex ) const						 // :252-255
	{
		const uint32_t c = attrs()[vIndex].x;
		return make_uchar4( c & 0xFF, ( c >> 8 ) & 0xFF, ( c >> 16 ) & 0xFF, ( c >> 24 ) & 0xFF );
	}
	__device__ float3 getVoxelEmission( uint32_t vIndex, bool withScale ) const // :256-259 (rawReflectance, renderCommon.hpp:160-166)
	{
		MVRT_DEVICE_FP_STRICT
		const uint32_t e = attrs()[vIndex].y;
		const float s = withScale ? view.emissionScale : 1.0f;
		return make_float3( (float)( e & 0xFF ) / 255.0f * s, (float)( ( e >> 8 ) & 0xFF ) / 255.0f * s, (float)( ( e >> 16 ) & 0xFF ) / 255.0f * s );
	}

	__device__ void intersect( float3 ro, float3 rd, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay ) const
	{
		StackEntry stack[MVRT_DEVICE_MAX_LEVELS];
		uint32_t descents;
		intersectEx( stack, ro, rd, t, nMajor, vIndex, isShadowRay, &descents );
	}
	__device__ void intersect( StackEntry* stack, float3 ro, float3 rd, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay ) const
	{
		uint32_t descents;
		intersectEx( stack, ro, rd, t, nMajor, vIndex, isShadowRay, &descents );
	}
	__device__ void intersectEx( float3 ro, float3 rd, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay, uint32_t* descents ) const
	{
		StackEntry stack[MVRT_DEVICE_MAX_LEVELS];
		intersectEx( stack, ro, rd, t, nMajor, vIndex, isShadowRay, descents );
	}
	// stack: view.levels entries (slot = tree level of the saved node)
	__device__ void intersectEx( StackEntry* stack, float3 ro, float3 rd, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay, uint32_t* descentsOut ) const
	{
		walk<false>( stack, ro, rd, 0.0f, t, nMajor, vIndex, isShadowRay, descentsOut );
	}

	// the same ray limited to t <= tMax
	__device__ void intersectRange( float3 ro, float3 rd, float tMax, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay ) const
	{
		StackEntry stack[MVRT_DEVICE_MAX_LEVELS];
		uint32_t descents;
		walk<true>( stack, ro, rd, tMax, t, nMajor, vIndex, isShadowRay, &descents );
	}
	__device__ void intersectRange( StackEntry* stack, float3 ro, float3 rd, float tMax, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay ) const
	{
		uint32_t descents;
		walk<true>( stack, ro, rd, tMax, t, nMajor, vIndex, isShadowRay, &descents );
	}
	__device__ void intersectRangeEx( float3 ro, float3 rd, float tMax, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay, uint32_t* descents ) const
	{
		StackEntry stack[MVRT_DEVICE_MAX_LEVELS];
		walk<true>( stack, ro, rd, tMax, t, nMajor, vIndex, isShadowRay, descents );
	}
	__device__ void intersectRangeEx( StackEntry* stack, float3 ro, float3 rd, float tMax, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay,
									  uint32_t* descents ) const
	{
		walk<true>( stack, ro, rd, tMax, t, nMajor, vIndex, isShadowRay, descents );
	}
	// a shadow ray with the limit: is anything hit with t <= tMax
	__device__ bool occluded( float3 ro, float3 rd, float tMax ) const
	{
		float t;
		int nMajor;
		uint32_t vIndex;
		intersectRange( ro, rd, tMax, &t, &nMajor, &vIndex, true );
		return t != detail::kMaxFloat;
	}
	__device__ bool occluded( StackEntry* stack, float3 ro, float3 rd, float tMax ) const
	{
		float t;
		int nMajor;
		uint32_t vIndex;
		intersectRange( stack, ro, rd, tMax, &t, &nMajor, &vIndex, true );
		return t != detail::kMaxFloat;
	}

	// The cone-limited ray (see the head of this file): level = the depth the walk stopped at (view.levels at a voxel), cellCode = the 3-bits-per-level path to
	// that cell = the Morton code of any voxel below it >> 3 * ( levels - level ).  A miss reports MVRT_MAX_FLOAT, -1, 0, 0
	__device__ void intersectCone( float3 ro, float3 rd, float coneA, float coneB, float* t, int* nMajor, uint32_t* level, uint64_t* cellCode ) const
	{
		StackEntry stack[MVRT_DEVICE_MAX_LEVELS];
		uint32_t descents;
		intersectConeEx( stack, ro, rd, coneA, coneB, t, nMajor, level, cellCode, &descents );
	}
	__device__ void intersectCone( StackEntry* stack, float3 ro, float3 rd, float coneA, float coneB, float* t, int* nMajor, uint32_t* level, uint64_t* cellCode ) const
	{
		uint32_t descents;
		intersectConeEx( stack, ro, rd, coneA, coneB, t, nMajor, level, cellCode, &descents );
	}
	__device__ void intersectConeEx( float3 ro, float3 rd, float coneA, float coneB, float* t, int* nMajor, uint32_t* level, uint64_t* cellCode, uint32_t* descents ) const
	{
		StackEntry stack[MVRT_DEVICE_MAX_LEVELS];
		intersectConeEx( stack, ro, rd, coneA, coneB, t, nMajor, level, cellCode, descents );
	}
	__device__ void intersectConeEx( StackEntry* stack, float3 ro, float3 rd, float coneA, float coneB, float* t, int* nMajor, uint32_t* level, uint64_t* cellCode,
									 uint32_t* descents ) const
	{
		uint32_t vIndex;
		walk<false, true>( stack, ro, rd, 0.0f, t, nMajor, &vIndex, false, descents, coneA, coneB, level, cellCode );
	}

	// the walk of every method above.  RANGE = false is the unlimited ray: tMax is not read and no compare is added to the loop
	template <bool RANGE>
	__device__ void walk( StackEntry* stack, float3 ro, float3 rd, float tMax, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay, uint32_t* descentsOut ) const
	{
		walk<RANGE, false>( stack, ro, rd, tMax, t, nMajor, vIndex, isShadowRay, descentsOut, 0.0f, 0.0f, nullptr, nullptr );
	}
	// ... with its second flag: CONE = true is the cone-limited ray (intersectCone).  coneA, coneB, levelOut and codeOut are read and written by it alone, and
	// its vIndex stays 0 (DeviceLod::lookup gives the index); CONE = false adds nothing to the loop
	template <bool RANGE, bool CONE>
	__device__ void walk( StackEntry* stack, float3 ro, float3 rd, float tMax, float* t, int* nMajor, uint32_t* vIndex, bool isShadowRay, uint32_t* descentsOut, float coneA,
						  float coneB, uint32_t* levelOut, uint64_t* codeOut ) const
	{
		MVRT_DEVICE_FP_STRICT
		using namespace detail;
		const bool embedded = view.flavour == MVRT_FLAVOUR_EMBEDDED;
		const float lox = view.lower[0], loy = view.lower[1], loz = view.lower[2];
		const float hix = view.upper[0], hiy = view.upper[1], hiz = view.upper[2];
		*t = kMaxFloat;
		*nMajor = -1;
		*vIndex = 0;
		*descentsOut = 0;
		if( CONE )
		{
			*levelOut = 0;
			*codeOut = 0;
		}
		if( RANGE && !( 0.0f < tMax ) ) return; // a hit has 0 < t: nothing lies within such a limit (NaN included)
		// ray setup, voxCommon.hpp:240-278
		float ix = 1.0f / rd.x, iy = 1.0f / rd.y, iz = 1.0f / rd.z;
		uint32_t vMask = 0;
		if( ix < 0.0f )
		{
			vMask |= 1u;
			ix = -ix;
			ro.x = lox + hix - ro.x;
		}
		if( iy < 0.0f )
		{
			vMask |= 2u;
			iy = -iy;
			ro.y = loy + hiy - ro.y;
		}
		if( iz < 0.0f )
		{
			vMask |= 4u;
			iz = -iz;
			ro.z = loz + hiz - ro.z;
		}
		ix = smin( ix, kMaxFloat / smax( smax( sabs( lox - ro.x ), sabs( hix - ro.x ) ), 1.0f ) );
		iy = smin( iy, kMaxFloat / smax( smax( sabs( loy - ro.y ), sabs( hiy - ro.y ) ), 1.0f ) );
		iz = smin( iz, kMaxFloat / smax( smax( sabs( loz - ro.z ), sabs( hiz - ro.z ) ), 1.0f ) );
		const float t0x = ( lox - ro.x ) * ix, t0y = ( loy - ro.y ) * iy, t0z = ( loz - ro.z ) * iz;
		float tx1 = ( hix - ro.x ) * ix, ty1 = ( hiy - ro.y ) * iy, tz1 = ( hiz - ro.z ) * iz;
		if( min3( tx1, ty1, tz1 ) < max3( t0x, t0y, t0z ) ) return; // misses the root box
		const float dtx = tx1 - t0x, dty = ty1 - t0y, dtz = tz1 - t0z; // :312
		// RANGE: the walk ends at the first candidate child entered later than `cut` = tMax + margin.  The entry times are recomputed per level, so a
		// voxel's t can lie below the entry time of a node visited before it: the margin, 16 (levels + 2)^2 roundings of the largest slab time, bounds
		// that.  Rays with a slab delta that is not finite (no front-to-back order) or with slab times whose sums could overflow are
		// never cut: +inf
		float cut = __uint_as_float( 0x7F800000u );
		if( RANGE )
		{
			const bool regular = ( __float_as_uint( dtx ) & 0x7F800000u ) != 0x7F800000u && ( __float_as_uint( dty ) & 0x7F800000u ) != 0x7F800000u &&
								 ( __float_as_uint( dtz ) & 0x7F800000u ) != 0x7F800000u;
			if( regular )
			{
				const float T = smax( smax( max3( sabs( t0x ), sabs( t0y ), sabs( t0z ) ), max3( sabs( tx1 ), sabs( ty1 ), sabs( tz1 ) ) ), 7.8886090522e-31f /* 2^-100 */ );
				const float k = (float)( 16u * ( view.levels + 2u ) * ( view.levels + 2u ) ) * 5.9604644775e-8f /* 2^-24 */;
				if( T <= 1.2676506002e+30f /* 2^100 */ ) cut = tMax + T * k;
			}
		}

		const detail::Line64* const lines = (const detail::Line64*)(uintptr_t)view.nodes;
		const uint32_t* const kids = (const uint32_t*)(uintptr_t)view.kids;
		const uint8_t* const masks = (const uint8_t*)(uintptr_t)view.masks;
		uint32_t node = embedded ? ( view.rootIndex | ( view.rootMask << 24 ) ) : view.rootIndex; // :306
		uint32_t nodeMask = view.rootMask;																	 // plain flavour: mask of the current node
		uint32_t level = 0, childMask = 8u /* first visit */, pending = 0, descents = 0;
		uint64_t resume = 0; // 3 bits per pending level: the candidate a popped node resumes with
		uint64_t path = 0;	 // child indices root -> current node, 3 bits per level
		const float rootEdge = CONE ? view.dps * __uint_as_float( ( 127u + view.levels ) << 23 ) : 0.0f; // dps * 2^levels
		for( ;; )
		{
			const float scale = __uint_as_float( ( 127u - level ) << 23 ); // 2^-level
			const float tx0 = tx1 - dtx * scale;							   // :317-320
			const float ty0 = ty1 - dty * scale;
			const float tz0 = tz1 - dtz * scale;
			const float S = max3( tx0, ty0, tz0 );
			bool pop = false;
			if( node == kLeaf ) // :322-334
			{
				if( 0.0f < S )
				{
					*descentsOut = descents;
					if( RANGE && !( S <= tMax ) ) return; // the unlimited ray's hit lies beyond the limit: a miss
					*t = S;
					*nMajor = ( S == tx0 ) ? 1 : ( ( S == ty0 ) ? 2 : 0 );
					if( CONE )
					{
						*levelOut = level;
						*codeOut = path;
					}
					else if( !isShadowRay )
						*vIndex = voxelIndexFromPath( path );
					return;
				}
				pop = true;
			}
			else
			{
				// CONE: an inner node below the root, entered in front of the origin and no larger than the ray's footprint there, is solid: it reports
				// the hit a voxel in its place would.  Tested on the first visit only, never after a pop
				if( CONE && ( childMask & 8u ) && level != 0u && level < view.levels )
				{
					const float f = coneA + coneB * S;
					if( 0.0f < S && rootEdge * scale <= f ) // (false for a NaN or negative f)
					{
						*descentsOut = descents;
						*t = S;
						*nMajor = ( S == tx0 ) ? 1 : ( ( S == ty0 ) ? 2 : 0 );
						*levelOut = level;
						*codeOut = path;
						return;
					}
				}
				const float txM = 0.5f * ( tx0 + tx1 ); // :338-340
				const float tyM = 0.5f * ( ty0 + ty1 );
				const float tzM = 0.5f * ( tz0 + tz1 );
				if( childMask & 8u ) childMask = ( txM < S ? 1u : 0u ) | ( tyM < S ? 2u : 0u ) | ( tzM < S ? 4u : 0u ); // :342-348
				const float x1 = ( childMask & 1u ) ? tx1 : txM;															   // :358-360
				const float y1 = ( childMask & 2u ) ? ty1 : tyM;
				const float z1 = ( childMask & 4u ) ? tz1 : tzM;
				const float u = min3( x1, y1, z1 ); // :364-372
				const uint32_t mv = ( u == x1 ) ? 1u : ( ( u == y1 ) ? 2u : 4u );
				const bool hasNext = ( childMask & mv ) == 0u;
				const uint32_t childIndex = childMask ^ vMask;
				const uint32_t nextMask = childMask | mv;
				const bool exists = embedded ? ( ( node >> ( 24u + childIndex ) ) & 1u ) != 0u : ( ( nodeMask >> childIndex ) & 1u ) != 0u;
				if( RANGE )
				{
					const float x0 = ( childMask & 1u ) ? txM : tx0, y0 = ( childMask & 2u ) ? tyM : ty0, z0 = ( childMask & 4u ) ? tzM : tz0;
					if( cut < max3( x0, y0, z0 ) ) break; // this child and every node still to come are entered beyond the limit
				}
				if( exists && !( u < 0.0f ) )
				{
					if( hasNext ) // push (:377-380)
					{
						StackEntry e;
						e.node = node;
						e.tx1 = tx1;
						e.ty1 = ty1;
						e.tz1 = tz1;
						stack[level] = e;
						pending |= 1u << level;
						resume = ( resume & ~( 7ull << ( 3u * level ) ) ) | ( (uint64_t)nextMask << ( 3u * level ) );
					}
					if( embedded ) // :381
					{
						const uint32_t n = node & 0xFFFFFFu;
						node = kids ? kids[n * 8u + childIndex] : lines[n].children[childIndex];
					}
					else
					{
						const detail::Line64* l = lines + node;
						nodeMask = ( l->psum[childIndex >> 2] >> ( 8u * ( childIndex & 3u ) ) ) & 0xFFu; // the child's mask, same line
						node = l->children[childIndex];
					}
					descents++;
					path = ( path << 3 ) | childIndex;
					tx1 = x1; // :382-386
					ty1 = y1;
					tz1 = z1;
					level++;
					childMask = 8u;
				}
				else if( hasNext )
					childMask = nextMask;
				else
					pop = true;
			}
			if( pop ) // :414-422
			{
				if( pending == 0u ) break;
				const uint32_t L = 31u - (uint32_t)__builtin_clz( pending );
				pending &= ~( 1u << L );
				const StackEntry e = stack[L];
				node = e.node;
				tx1 = e.tx1;
				ty1 = e.ty1;
				tz1 = e.tz1;
				childMask = (uint32_t)( resume >> ( 3u * L ) ) & 7u;
				path >>= 3u * ( level - L );
				level = L;
				if( !embedded ) nodeMask = masks[node];
			}
		}
		*descentsOut = descents;
	}

	// vIndex of the voxel at `path` = the stored nVoxelsPSum summed along root -> voxel (voxCommon.hpp:388-391)
	__device__ uint32_t voxelIndexFromPath( uint64_t path ) const
	{
		const detail::Line64* const lines = (const detail::Line64*)(uintptr_t)view.nodes;
		const uint32_t* const psumCold = (const uint32_t*)(uintptr_t)view.psumCold;
		const bool embedded = view.flavour == MVRT_FLAVOUR_EMBEDDED;
		uint32_t n = view.rootIndex, v = 0;
		for( uint32_t l = 0; l < view.levels; l++ )
		{
			const uint32_t c = (uint32_t)( path >> ( 3u * ( view.levels - 1u - l ) ) ) & 7u;
			if( embedded )
			{
				v += lines[n].psum[c];
				n = lines[n].children[c] & 0xFFFFFFu;
			}
			else
			{
				v += psumCold[(uint64_t)n * 8u + c];
				n = lines[n].children[c];
			}
		}
		return v;
	}

private:
	__device__ const uint2* attrs() const { return (const uint2*)(uintptr_t)view.attrs; }
};

// The attribute pyramid of an octree (mvrt_svo_lod_prepare, mvrt_svo_lod_view): per level the occupied cells as ascending codes, with their mean attributes.
// The octree is a DAG -- subtrees of equal shape share their nodes whatever their colours --, so attributes are keyed by the cell's code, not by the node
struct DeviceLod
{
	mvrt_device_lod view;

	DeviceLod() = default;
	__host__ __device__ explicit DeviceLod( const mvrt_device_lod& v ) : view( v ) {}

	// the rank of cellCode among the cells of `level` in [1, view.levels] (binary search); false when the level holds no such cell.  At level == view.levels the
	// rank is the voxel's vIndex
	__host__ __device__ bool lookup( uint32_t level, uint64_t cellCode, uint32_t* index ) const
	{
		if( level == 0u || level > view.levels ) return false;
		const uint64_t* const codes = (const uint64_t*)(uintptr_t)view.codes[level];
		uint32_t lo = 0, hi = view.count[level];
		while( lo < hi )
		{
			const uint32_t mid = lo + ( hi - lo ) / 2u;
			if( codes[mid] < cellCode ) lo = mid + 1u;
			else hi = mid;
		}
		if( lo == view.count[level] || codes[lo] != cellCode ) return false;
		*index = lo;
		return true;
	}
	// the 8-byte attribute {colour, emission} of cell `index` of `level`
	__host__ __device__ uint2 attrib( uint32_t level, uint32_t index ) const { return ( (const uint2*)(uintptr_t)view.attrs[level] )[index]; }
	__host__ __device__ uchar4 color( uint32_t level, uint32_t index ) const
	{
		const uint32_t c = attrib( level, index ).x;
		return make_uchar4( c & 0xFF, ( c >> 8 ) & 0xFF, ( c >> 16 ) & 0xFF, ( c >> 24 ) & 0xFF );
	}
};
} // namespace mvrt
