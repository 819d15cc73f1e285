// kernels_denoise.hip -- the luminance-moments buffer (mvrt_pt_set_moments) and the variance-guided a-trous denoiser (mvrt_denoise_buffers,
// mvrt_pt_denoise).  New; the reference has neither.  The filter is a CONTRACT (include/mvrt.h "Denoiser"): every operation below is fp32 in
// the order stated there, compiled without contraction, exp is mvrt_exp, division and sqrt are IEEE -- the test helper restates that text, not this file.
#include "../../include/mvrt.h"
#include "launch.h"

// lum( x ) = ( 0.2126 r + 0.7152 g ) + 0.0722 b: the one luminance of the moments, of the albedo normalisation and of the edge-stopping term
static MVRT_DI float lum3( float r, float g, float b ) { return ( 0.2126f * r + 0.7152f * g ) + 0.0722f * b; }

// ---- moments: moments[p].x += sum of l, .y += sum of l * l over the 16 samples of each merged step ---------------------------------------------------
// Reads the Ls* planes exactly as kPtAccumulate does (four 16-byte loads per plane, pixel and step) and adds in its order: per step the 16 samples ascending
// from +0, the product l * l rounded before it is added, then the two partial sums onto the buffer, steps in issue order.  z and w are never written.
static MVRT_DI uint64_t activePixel( uint64_t slot ) { return slot; }
static MVRT_DI uint64_t activePixel( uint64_t slot, const uint32_t* active ) { return active[slot]; }
// Under a sample mask: n = the active pixels, p = a slot of the active list, and the pixel's record is reached through the list as in kPtAccumulate.
// ACTIVE: empty, or the list (one `const uint32_t*`); the unmasked instantiation compiles to the instructions the kernel had without the mask.
template <class... ACTIVE>
__global__ void __launch_bounds__( 256 ) kPtMoments( const float* __restrict__ Lsx, const float* __restrict__ Lsy, const float* __restrict__ Lsz, uint64_t n, int nSteps,
													   float4* __restrict__ moments, ACTIVE... active )
{
	for( uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256 )
	{
		const uint64_t px = sizeof...( ACTIVE ) ? (uint64_t)activePixel( p, active... ) : p;
		float4 v = moments[px];
		for( int b = 0; b < nSteps; b++ )
		{
			const uint64_t base = ( (uint64_t)b * n + p ) * MVRT_SPP_PER_STEP;
			const float4* sx = (const float4*)( Lsx + base );
			const float4* sy = (const float4*)( Lsy + base );
			const float4* sz = (const float4*)( Lsz + base );
			float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
			for( int q = 0; q < MVRT_SPP_PER_STEP / 4; q++ )
			{
				const float4 vx = sx[q], vy = sy[q], vz = sz[q];
				const float l0 = lum3( vx.x, vy.x, vz.x ), l1 = lum3( vx.y, vy.y, vz.y ), l2 = lum3( vx.z, vy.z, vz.z ), l3 = lum3( vx.w, vy.w, vz.w );
				s1 += l0; s2 += l0 * l0;
				s1 += l1; s2 += l1 * l1;
				s1 += l2; s2 += l2 * l2;
				s1 += l3; s2 += l3 * l3;
			}
			v.x += s1;
			v.y += s2;
		}
		moments[px] = v;
	}
}
int launchPtMoments( const PtBuffers& buf, uint64_t validOwnedPixels, int nSteps, float4* moments, int nCUs, hipStream_t stream, const uint32_t* active )
{
	if( validOwnedPixels == 0 ) return 0;
	uint32_t grid = divUp( validOwnedPixels, 256 );
	if( nCUs > 0 && grid > (uint32_t)nCUs * 8u ) grid = (uint32_t)nCUs * 8u;
	if( active ) hipLaunchKernelGGL( kPtMoments<const uint32_t*>, dim3( grid ), dim3( 256 ), 0, stream, buf.Lsx, buf.Lsy, buf.Lsz, validOwnedPixels, nSteps, moments, active );
	else hipLaunchKernelGGL( kPtMoments<>, dim3( grid ), dim3( 256 ), 0, stream, buf.Lsx, buf.Lsy, buf.Lsz, validOwnedPixels, nSteps, moments );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// ---- error mask (mvrt_pt_error_mask): which pixels have not converged ---------------------------------------------------------------------------------
// A CONTRACT like the filter (include/mvrt.h "Adaptive sampling"): se = sqrt( var ) with the denoiser's var, active iff se > threshold * max( m1, lumFloor ),
// fp32 in that order.  One lane per owned pixel, one byte each (padding 0); the ones are counted per wave with one atomic.
__global__ void __launch_bounds__( 256 ) kErrorMask( const float4* __restrict__ fb, const float4* __restrict__ moments, uint64_t nValid, uint64_t nOwned, float threshold, float lumFloor,
													   float minSamples, float maxSamples, uint8_t* __restrict__ mask, uint32_t* __restrict__ count )
{
	const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	bool on = false;
	if( p < nValid )
	{
		const float n = fb[p].w;
		if( n < minSamples ) on = true; // (n == 0 among them)
		else if( maxSamples > 0.0f && n >= maxSamples ) on = false;
		else
		{
			const float4 m4 = moments[p];
			const float m1 = m4.x / n, m2 = m4.y / n;
			const float var = smax( m2 - m1 * m1, 0.0f ) / smax( n - 1.0f, 1.0f );
			const float se = sqrtf( var );
			on = se > threshold * smax( m1, lumFloor );
		}
	}
	if( p < nOwned ) mask[p] = on ? 1 : 0;
	const unsigned long long b = __ballot( on );
	if( ( threadIdx.x & 63u ) == 0 && b ) atomicAdd( count, (uint32_t)__popcll( b ) );
}
int launchErrorMask( const float4* frameBuffer, const float4* moments, uint64_t validOwnedPixels, uint64_t ownedPixels, float threshold, float lumFloor, int minSamples,
					 int maxSamples, uint8_t* mask, uint32_t* countDev, hipStream_t stream )
{
	MVRT_HIP( hipMemsetAsync( countDev, 0, 4, stream ) );
	hipLaunchKernelGGL( kErrorMask, dim3( divUp( ownedPixels, 256 ) ), dim3( 256 ), 0, stream, frameBuffer, moments, validOwnedPixels, ownedPixels, threshold, lumFloor, (float)minSamples,
						(float)maxSamples, mask, countDev );
	MVRT_HIP( hipGetLastError() );
	return 0;
}

// ---- denoiser ---------------------------------------------------------------------------------------------------------------------------------------
// What a tap reads of a pixel: two 16-byte records and one float.
//   uv  { u.xyz, v }   demodulated mean radiance and the variance of its luminance; ping-ponged across the iterations
//   geo { N.xyz, Z }   mean first-hit normal and mean hit t: a caller's values, of any sign
//   cov f = h / n      hit share.  f = DN_NO_TAP marks a pixel that is never filtered and never a tap -- sky (h == 0) or without samples (n == 0).  The
//                      marker is negative and h / n of a filtered pixel (n > 0 and h > 0) never is, whatever the other buffers hold, so validity is what the
//                      contract says and nothing else; a tap is rejected on the float it loads anyway
#define DN_NO_TAP -1.0f
#define DN_TILE_X 32
#define DN_TILE_Y 8

// A_k = max( ( albedo_k + ( n - h ) ) / n, floor ): misses count as albedo 1
static MVRT_DI f3 dnAlbedo( float4 albedo, float n, float floorA, uint32_t flags )
{
	if( flags & 1u ) return mk3( 1.0f, 1.0f, 1.0f );
	const float miss = n - albedo.w;
	return mk3( smax( ( albedo.x + miss ) / n, floorA ), smax( ( albedo.y + miss ) / n, floorA ), smax( ( albedo.z + miss ) / n, floorA ) );
}

__global__ void __launch_bounds__( 256 ) kDenoisePrepare( const float4* __restrict__ color, const float4* __restrict__ albedo, const float4* __restrict__ normalDepth,
															const float4* __restrict__ moments, uint32_t nPixels, float floorA, uint32_t flags, float4* __restrict__ uv,
															float4* __restrict__ geo, float* __restrict__ cov, float4* __restrict__ out )
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if( p >= nPixels ) return;
	const float4 c4 = color[p], a4 = albedo[p];
	const float n = c4.w, h = a4.w;
	if( n == 0.0f )
	{
		uv[p] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
		geo[p] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
		cov[p] = DN_NO_TAP;
		out[p] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
		return;
	}
	const f3 c = mk3( c4.x / n, c4.y / n, c4.z / n );
	if( h == 0.0f ) // sky: passed through exactly
	{
		uv[p] = make_float4( c.x, c.y, c.z, 0.0f );
		geo[p] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
		cov[p] = DN_NO_TAP;
		out[p] = make_float4( c.x, c.y, c.z, 1.0f );
		return;
	}
	const float4 g4 = normalDepth[p], m4 = moments[p];
	const f3 A = dnAlbedo( a4, n, floorA, flags );
	const float m1 = m4.x / n, m2 = m4.y / n;
	const float var = smax( m2 - m1 * m1, 0.0f ) / smax( n - 1.0f, 1.0f );
	const float lA = lum3( A.x, A.y, A.z );
	uv[p] = make_float4( c.x / A.x, c.y / A.y, c.z / A.z, var / ( lA * lA ) );
	geo[p] = make_float4( g4.x / n, g4.y / n, g4.z / n, g4.w / h );
	cov[p] = h / n;
	// (out[p] is written by the last iteration)
}

struct DnSigmas
{
	float n2;  // sigmaNormal * sigmaNormal
	float z, f, l;
};

// what the centre pixel contributes to every tap, and the running sums of the contract
struct DnCentre
{
	float4 g; // { N.xyz, Z }
	float f, l, sv;
};
struct DnSums
{
	float ax, ay, az, av, ws;
};
// one tap, the operations of the contract in its order; k = k[dy] * k[dx] (exact in fp32)
static MVRT_DI void dnTap( const DnCentre& c, const DnSigmas& sg, float k, float4 gq, float4 uq, float fq, DnSums& a )
{
	const float nx = c.g.x - gq.x, ny = c.g.y - gq.y, nz = c.g.z - gq.z;
	float e = ( ( nx * nx + ny * ny ) + nz * nz ) / sg.n2;
	const float dz = ( c.g.w - gq.w ) / ( sg.z * smax( smax( c.g.w, gq.w ), 1e-20f ) );
	e = e + dz * dz;
	const float df = ( c.f - fq ) / sg.f;
	e = e + df * df;
	e = e + sabs( c.l - lum3( uq.x, uq.y, uq.z ) ) / c.sv;
	const float w = k * mvrt_exp( -e );
	a.ax = a.ax + w * uq.x;
	a.ay = a.ay + w * uq.y;
	a.az = a.az + w * uq.z;
	a.av = a.av + ( w * w ) * uq.w;
	a.ws = a.ws + w;
}
static MVRT_DI float dnKernel( int d ) { return d == 0 ? 0.375f : ( d == -1 || d == 1 ? 0.25f : 0.0625f ); }
template <bool LAST>
static MVRT_DI void dnStore( const DnSums& a, uint32_t p, float4* __restrict__ uvOut, const float4* __restrict__ color, const float4* __restrict__ albedo, float floorA, uint32_t flags,
							 float4* __restrict__ out )
{
	const float ux = a.ax / a.ws, uy = a.ay / a.ws, uz = a.az / a.ws;
	if( LAST )
	{
		const f3 A = dnAlbedo( albedo[p], color[p].w, floorA, flags );
		out[p] = make_float4( ux * A.x, uy * A.y, uz * A.z, 1.0f );
	}
	else uvOut[p] = make_float4( ux, uy, uz, a.av / ( a.ws * a.ws ) );
}

// One a-trous iteration, plain gather: one lane per pixel, 25 taps of stride s in the order of the contract (dy outer, dx inner), each tap two 16-byte loads
// and one 4-byte load, all of them L2 / Infinity Cache hits at the frame sizes this runs on (an LDS-staged variant measured no faster: DESIGN.md 5.8).  LAST: writes out = { u' * A, 1 } instead of the next { u', v' }.
template <bool LAST>
__global__ void __launch_bounds__( 256 ) kDenoiseAtrous( const float4* __restrict__ uvIn, const float4* __restrict__ geo, const float* __restrict__ cov, int W, int H, int s, DnSigmas sg,
														   float4* __restrict__ uvOut, const float4* __restrict__ color, const float4* __restrict__ albedo, float floorA, uint32_t flags,
														   float4* __restrict__ out )
{
	const int x = (int)( blockIdx.x * DN_TILE_X + ( threadIdx.x % DN_TILE_X ) ), y = (int)( blockIdx.y * DN_TILE_Y + ( threadIdx.x / DN_TILE_X ) );
	if( x >= W || y >= H ) return;
	const uint32_t p = (uint32_t)y * (uint32_t)W + (uint32_t)x;
	DnCentre c;
	c.f = cov[p];
	if( c.f < 0.0f ) return; // sky or empty: prepare wrote the output, and no tap ever reads this pixel's record
	c.g = geo[p];
	const float4 up = uvIn[p];
	c.l = lum3( up.x, up.y, up.z );
	c.sv = sg.l * sqrtf( up.w ) + 1e-6f;
	DnSums a = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
	for( int dy = -2; dy <= 2; dy++ )
	{
		const int qy = y + dy * s;
#pragma unroll
		for( int dx = -2; dx <= 2; dx++ )
		{
			const int qx = x + dx * s;
			if( qx < 0 || qx >= W || qy < 0 || qy >= H ) continue;
			const uint32_t q = (uint32_t)qy * (uint32_t)W + (uint32_t)qx;
			const float fq = cov[q];
			if( fq < 0.0f ) continue;
			dnTap( c, sg, dnKernel( dy ) * dnKernel( dx ), geo[q], uvIn[q], fq, a );
		}
	}
	dnStore<LAST>( a, p, uvOut, color, albedo, floorA, flags, out );
}

static uint64_t dnAlign( uint64_t b ) { return ( b + 255 ) & ~(uint64_t)255; }
uint64_t denoiseScratchBytes( uint64_t nPixels ) { return 3 * dnAlign( nPixels * 16 ) + dnAlign( nPixels * 4 ); }

// arguments are checked by the callers (api_pt.hip); scratch holds denoiseScratchBytes( W * H )
int launchDenoise( const float4* color, const float4* albedo, const float4* normalDepth, const float4* moments, int W, int H, const mvrt_denoise_params& p, float4* out, void* scratch,
				   hipStream_t stream )
{
	const uint64_t n = (uint64_t)W * H;
	uint8_t* base = (uint8_t*)scratch;
	float4* uv[2] = { (float4*)base, (float4*)( base + dnAlign( n * 16 ) ) };
	float4* geo = (float4*)( base + 2 * dnAlign( n * 16 ) );
	float* cov = (float*)( base + 3 * dnAlign( n * 16 ) );
	hipLaunchKernelGGL( kDenoisePrepare, dim3( divUp( n, 256 ) ), dim3( 256 ), 0, stream, color, albedo, normalDepth, moments, (uint32_t)n, p.albedoFloor, p.flags, uv[0], geo, cov, out );
	const DnSigmas sg = { p.sigmaNormal * p.sigmaNormal, p.sigmaDepth, p.sigmaCoverage, p.sigmaLuminance };
	const dim3 grid( divUp( W, DN_TILE_X ), divUp( H, DN_TILE_Y ) );
	for( int i = 0; i < p.iterations; i++ )
	{
		const float4* in = uv[i & 1];
		float4* next = uv[( i & 1 ) ^ 1];
		if( i + 1 < p.iterations )
			hipLaunchKernelGGL( kDenoiseAtrous<false>, grid, dim3( 256 ), 0, stream, in, geo, cov, W, H, 1 << i, sg, next, color, albedo, p.albedoFloor, p.flags, out );
		else
			hipLaunchKernelGGL( kDenoiseAtrous<true>, grid, dim3( 256 ), 0, stream, in, geo, cov, W, H, 1 << i, sg, next, color, albedo, p.albedoFloor, p.flags, out );
	}
	MVRT_HIP( hipGetLastError() );
	return 0;
}
