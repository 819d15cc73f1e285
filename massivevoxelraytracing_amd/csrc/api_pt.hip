// api_pt.hip -- the C-ABI of libmvrt_hip.so (include/mvrt.h), second half: the path tracer (the reference's host struct PathTracer, PathTracer.hpp:14-170,
// behind an opaque handle), its feature buffers, moments and denoiser, and the RGBE reader.  It meets api.hip in the octree handle (api_handles.h) and needs
// nothing of the traversal's device code.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "api_handles.h"

// ---- PMJ02 table (host), pmjSampler.hpp:14-58,114-144 -----------------------------------------------------
namespace
{
struct PCG32 // renderCommon.hpp:86-110
{
	uint64_t state, inc;
	void setup( uint64_t seed, uint64_t stream )
	{
		state = 0;
		inc = stream * 2 + 1;
		nextU32();
		state += seed;
		nextU32();
	}
	uint32_t nextU32()
	{
		uint64_t old = state;
		state = old * 6364136223846793005ULL + inc;
		uint32_t xs = (uint32_t)( ( ( old >> 18u ) ^ old ) >> 27u );
		uint32_t rot = (uint32_t)( old >> 59u );
		return ( xs >> rot ) | ( xs << ( ( -rot ) & 31 ) );
	}
};
inline float uniformf( uint32_t x ) { return mvrt_u2f( ( x >> 9 ) | 0x3f800000u ) - 1.0f; } // :112-117

// Helmer's stochastic generation of a pmj02 sequence; xi0 is drawn before xi1 (see DESIGN.md "PMJ order")
void pmj02Sequence( int numSamples, float* samples, PCG32& rng )
{
	static const uint32_t xors[2][32] = {
		{ 0x0, 0x0, 0x2, 0x6, 0x6, 0xe, 0x36, 0x4e, 0x16, 0x2e, 0x276, 0x6ce, 0x716, 0xc2e, 0x3076, 0x40ce, 0x116, 0x22e, 0x20676, 0x60ece, 0x61716,
		  0xe2c2e, 0x367076, 0x4ec0ce, 0x170116, 0x2c022e, 0x2700676, 0x6c00ece, 0x7001716, 0xc002c2e, 0x30007076, 0x4000c0ce },
		{ 0x0, 0x1, 0x3, 0x3, 0x7, 0x1b, 0x27, 0xb, 0x17, 0x13b, 0x367, 0x38b, 0x617, 0x183b, 0x2067, 0x8b, 0x117, 0x1033b, 0x30767, 0x30b8b,
		  0x71617, 0x1b383b, 0x276067, 0xb808b, 0x160117, 0x138033b, 0x3600767, 0x3800b8b, 0x6001617, 0x1800383b, 0x20006067, 0x808b } };
	samples[0] = uniformf( rng.nextU32() );
	samples[1] = uniformf( rng.nextU32() );
	for( int logN = 0; ( 1 << logN ) < numSamples; logN++ )
	{
		const int prevLen = 1 << logN;
		const int nStrata = prevLen * 2;
		const float iStrata = 1.0f / nStrata;
		for( int i = 0; i < prevLen && ( prevLen + i ) < numSamples; i++ )
		{
			const int xStratum = ( (int)( samples[( i ^ xors[0][logN] ) * 2] * nStrata ) ) ^ 1;
			const int yStratum = ( (int)( samples[( i ^ xors[1][logN] ) * 2 + 1] * nStrata ) ) ^ 1;
			const float xi0 = uniformf( rng.nextU32() );
			const float xi1 = uniformf( rng.nextU32() );
			samples[( prevLen + i ) * 2] = ( xi0 + xStratum ) * iStrata;
			samples[( prevLen + i ) * 2 + 1] = ( xi1 + yStratum ) * iStrata;
		}
	}
}

// Radiance RGBE reader: header lines, blank line, "-Y h +X w", then flat or new-RLE scanlines.
int loadRgbe( const char* path, std::vector<float>& rgba, int* w, int* h )
{
	FILE* fp = fopen( path, "rb" );
	REQUIRE( fp, "cannot open %s", path );
	std::vector<uint8_t> d;
	uint8_t tmp[65536];
	size_t got;
	while( ( got = fread( tmp, 1, sizeof( tmp ), fp ) ) > 0 ) d.insert( d.end(), tmp, tmp + got );
	fclose( fp );
	size_t pos = 0;
	bool blank = false;
	*w = *h = 0;
	while( pos < d.size() )
	{
		size_t e = pos;
		while( e < d.size() && d[e] != '\n' ) e++;
		std::string line( (const char*)d.data() + pos, e - pos );
		pos = e + 1;
		if( !blank )
		{
			if( line.empty() ) blank = true;
			continue;
		}
		REQUIRE( sscanf( line.c_str(), "-Y %d +X %d", h, w ) == 2, "%s: unsupported resolution line '%s'", path, line.c_str() );
		break;
	}
	REQUIRE( *w > 0 && *h > 0, "%s: not a Radiance .hdr file", path );
	const int W = *w, H = *h;
	rgba.resize( (size_t)W * H * 4 );
	std::vector<uint8_t> scan( (size_t)W * 4 );
	for( int y = 0; y < H; y++ )
	{
		if( pos + 4 <= d.size() && W >= 8 && W < 32768 && d[pos] == 2 && d[pos + 1] == 2 && ( d[pos + 2] & 0x80 ) == 0 && ( ( d[pos + 2] << 8 ) | d[pos + 3] ) == W )
		{
			pos += 4;
			for( int c = 0; c < 4; c++ )
			{
				int x = 0;
				while( x < W )
				{
					REQUIRE( pos < d.size(), "%s: truncated RLE data", path );
					int count = d[pos++];
					if( count > 128 )
					{
						count -= 128;
						REQUIRE( pos < d.size() && x + count <= W, "%s: bad RLE run", path );
						uint8_t v = d[pos++];
						for( int k = 0; k < count; k++ ) scan[( x++ ) * 4 + c] = v;
					}
					else
					{
						REQUIRE( pos + count <= d.size() && x + count <= W, "%s: bad RLE literal", path );
						for( int k = 0; k < count; k++ ) scan[( x++ ) * 4 + c] = d[pos++];
					}
				}
			}
		}
		else
		{
			REQUIRE( pos + (size_t)W * 4 <= d.size(), "%s: truncated pixel data", path );
			memcpy( scan.data(), d.data() + pos, (size_t)W * 4 );
			pos += (size_t)W * 4;
		}
		for( int x = 0; x < W; x++ )
		{
			const uint8_t* p = &scan[(size_t)x * 4];
			float* o = &rgba[( (size_t)y * W + x ) * 4];
			if( p[3] )
			{
				float f = mvrt_u2f( (uint32_t)( (int)p[3] - 136 + 127 ) << 23 ); // 2^(E-136), E >= 10 keeps it normal
				if( (int)p[3] - 136 + 127 <= 0 ) f = 0.0f;
				o[0] = p[0] * f;
				o[1] = p[1] * f;
				o[2] = p[2] * f;
			}
			else
			{
				o[0] = o[1] = o[2] = 0.0f;
			}
			o[3] = 1.0f;
		}
	}
	return 0;
}
} // namespace

// ---- PathTracer ---------------------------------------------------------------------------------------------
struct EventProfiler : PtProfiler
{
	struct Rec
	{
		hipEvent_t a, b;
		int cls;
	};
	std::vector<Rec> recs;
	std::vector<hipEvent_t> pool;
	double ms[3] = { 0, 0, 0 };
	uint64_t traceLaunches = 0;
	hipEvent_t get()
	{
		if( !pool.empty() )
		{
			hipEvent_t e = pool.back();
			pool.pop_back();
			return e;
		}
		hipEvent_t e;
		(void)hipEventCreate( &e );
		return e;
	}
	void begin( int cls, hipStream_t s ) override
	{
		Rec r;
		r.a = get();
		r.b = get();
		r.cls = cls;
		(void)hipEventRecord( r.a, s );
		recs.push_back( r );
	}
	void end( hipStream_t s ) override { (void)hipEventRecord( recs.back().b, s ); }
	void collect() // caller has synchronised the stream
	{
		for( Rec& r : recs )
		{
			float t = 0.0f;
			if( hipEventElapsedTime( &t, r.a, r.b ) == hipSuccess ) ms[r.cls] += t;
			if( r.cls == MVRT_K_TRACE ) traceLaunches++;
			pool.push_back( r.a );
			pool.push_back( r.b );
		}
		recs.clear();
	}
	~EventProfiler()
	{
		collect();
		for( hipEvent_t e : pool ) (void)hipEventDestroy( e );
	}
};

struct mvrt_pt
{
	mvrt_svo* intersector = nullptr; // m_intersectorOctreeGPU
	DevBuf pmj;						 // m_pmj
	struct Hdri // m_hdri: what the kernels take by value and the buffers behind it.  Replaced as a whole by a successful load
	{
		DevBuf pixels, primary, sat[7];
		HdriDev dev = {};
	};
	Hdri hdri;
	// One frame: its sizes and every buffer sized by them.  A handle has a whole frame -- these buffers as far as the options ask for them, and the path state of
	// `depth` slots -- or none (f32.p == nullptr, every size 0: forgetFrame), which every entry point that reads a frame refuses on the host.
	struct Frame
	{
		int width = 0, height = 0;
		uint64_t ownedPixels = 0, validOwnedPixels = 0;
		DevBuf f32, u8;					 // m_frameBufferF32 / m_frameBufferU8
		DevBuf albedo, normalDepth;		 // first-hit feature buffers (mvrt_pt_set_aovs): float4 per owned pixel like f32, allocated and cleared with it
		DevBuf moments;					 // luminance moments (mvrt_pt_set_moments), independent of the feature buffers: one more float4 per owned pixel
		DevBuf denoised, denoiseScratch; // mvrt_pt_denoise: its output (float4 per pixel of the frame) and its scratch, kept between calls
		// Sample mask (mvrt_pt_set_sample_mask).  masked: the steps issued from now on sample the nActive pixels of activeList (their local indices, ascending; one
		// uint32 per owned pixel).  The list may outlive `masked`: passes in flight still read it, so it goes with the frame or when the next list replaces it
		DevBuf activeList;
		uint64_t nActive = 0;
		bool masked = false;
		DevBuf errorCount; // mvrt_pt_error_mask: its counter
		const uint32_t* passList() const { return masked ? activeList.as<uint32_t>() : nullptr; }
		uint64_t activePixels() const { return masked ? nActive : validOwnedPixels; }
		void dropMask() // the caller has drained
		{
			activeList.release();
			nActive = 0;
			masked = false;
		}
		uint64_t accumBytes() const { return ownedPixels * sizeof( float4 ); }
		void release() { *this = Frame(); }
		void releaseDenoised() // alone: by a resize (an image of the old size) and by a denoise that failed
		{
			denoised.release();
			denoiseScratch.release();
		}
		int alloc( bool aovs, bool withMoments ) // for the sizes set before; a buffer that is held lets go of its block as its turn comes, not earlier
		{
			return f32.alloc( accumBytes() ) || u8.alloc( ownedPixels * sizeof( uchar4 ) ) || ( aovs && ( albedo.alloc( accumBytes() ) || normalDepth.alloc( accumBytes() ) ) ) ||
				   ( withMoments && moments.alloc( accumBytes() ) );
		}
		int clear( hipStream_t st ) // the accumulation buffers that exist
		{
			for( DevBuf* b : { &f32, &albedo, &normalDepth, &moments } )
				if( b->p ) MVRT_HIP( hipMemsetAsync( b->p, 0, b->bytes, st ) );
			return 0;
		}
	};
	Frame frame;
	bool aovs = false, moments = false; // the options (off by default): they outlive a frame, the next successful resize allocates their buffers again
	int steps = 0;
	int tileIndex = 0, tileCount = 1;
	// wavefront work buffers: one set per in-flight step.  Consecutive step() calls are pipelined on internal
	// streams (depth slots) so that the thin late bounces of one step overlap the dense early bounces of the next;
	// the frame-buffer additions stay in step order through an event chain.  depth 1 = everything on the caller's stream.
	struct Slot
	{
		DevBuf work, dbg;
		DevBuf aovPart; // feature buffers on: the pass's partial sums, 2 x float4 per (step, pixel) (AovBuffers::partA / partN)
		PtBuffers buf;
		Workspace trace;
		hipStream_t stream = nullptr;
		hipEvent_t accumDone = nullptr;
		Slot() { memset( &buf, 0, sizeof( buf ) ); }
		void release() // no path state: cap = 0, so launchPass refuses to run, and no pointer into the freed block is left
		{
			work.release();
			aovPart.release();
			memset( &buf, 0, sizeof( buf ) );
		}
	};
	Slot slots[4];
	// deferred execution: up to `batch` consecutive step() calls are merged into ONE wavefront pass (bigger launches,
	// same per-sample results, frame-buffer additions still in step order).  Flushed by any consumer of the frame.
	std::vector<CameraPinhole> pendingCams;
	int pendingIteration = 0;
	hipStream_t pendingStream = nullptr;
	int batchCap = MVRT_MAX_BATCH; // footprint bound (allocWork)
	int batch = 0; // 0 = automatic: merge steps until a pass holds ~2 full-HD steps worth of samples (see effectiveBatch)
	int depth = 3;
	int depthWanted = 3; // what the caller asked for; `depth` may be lower when the path state would not fit (allocWork)
	int nextSlot = 0, lastSlot = 0;
	DevBuf statsBuf; // PtBuffers::stats of every slot (atomic tallies); allocated with the first frame and kept
	hipEvent_t forkEv = nullptr;
	hipEvent_t lastAccum = nullptr;
	bool pendingJoin = false;
	bool setupDone = false;
	bool profiling = false;
	uint64_t testFreeBytes = 0; // != 0: allocWork budgets against this instead of hipMemGetInfo (tests of the failure path)
	bool debugCapture = false; // keep the survivor list of every shade stage of the last pass (mvrt_pt_set_debug_capture)
	EventProfiler prof;
	int numCUs = 0;
	bool splitSmallPasses = true; // MVRT_SPLIT_SMALL=0 disables (A/B)
	bool originHints = true;	  // secondary rays start below the root (mvrt_pt_set_origin_hints)
	mvrt_pt()
	{
		hdri.dev.scale = 1.75f; // renderCommon.hpp:480
		depth = (int)mvrtKnob( "MVRT_PIPELINE_DEPTH", depth );
		if( depth < 1 ) depth = 1;
		if( depth > 4 ) depth = 4;
		depthWanted = depth;
		splitSmallPasses = mvrtKnob( "MVRT_SPLIT_SMALL", 1 ) != 0;
		batch = (int)mvrtKnob( "MVRT_BATCH_STEPS", 0 );
		if( batch < 0 ) batch = 0;
		if( batch > MVRT_MAX_BATCH ) batch = MVRT_MAX_BATCH;
	}
	int flush( bool moreStepsFollow = false ); // launch the pending steps
	int launchPass( const CameraPinhole* cams, int iteration, int nSteps, int traceGridDiv );
	int allocWorkSlot( Slot& sl );
	int allocSlots();
	// The one way to have no frame, and what every failed (re)allocation of a frame ends in, so that nothing stale is left behind: no slot has path state and the
	// frame is released with its sizes zeroed, so that the next resizeFrameBufferIfNeeded -- same size or not -- allocates again instead of returning early onto
	// freed memory.  No HIP call on a handle that holds nothing.  Returns 1, the status of the call that failed.
	int forgetFrame()
	{
		for( Slot& sl : slots ) sl.release();
		frame.release();
		return 1;
	}
	// (Re)allocates the path state of every pipeline slot, for the frame, the options, `batch` and `depthWanted` as they are now
	int allocWork() { return allocSlots() == 0 ? 0 : forgetFrame(); }
	int setOption( bool& flag, bool on, std::initializer_list<DevBuf*> bufs, std::initializer_list<DevBuf*> goWithThem, const char* who, const char* what );
	int effectiveBatch() const // merged steps per pass, bounded so that one pass stays below ~160 M samples (~30 GB of path state)
	{
		uint64_t perStep = frame.ownedPixels * MVRT_SPP_PER_STEP;
		if( perStep == 0 ) return 1;
		int b = batch;
		if( b == 0 ) // automatic: big enough to amortise launch tails, small enough that several passes can pipeline
		{
			b = (int)( ( 66000000ull + perStep / 2 ) / perStep );
			if( b < 1 ) b = 1;
			if( b > MVRT_MAX_BATCH ) b = MVRT_MAX_BATCH;
		}
		while( b > 1 && perStep * b > 160000000ull ) b--;
		if( b > batchCap ) b = batchCap; // lowered by allocWork when the path state would not fit the free HBM
		return b;
	}
	// steps merged into the next pass: effectiveBatch(), but at most HALF of the caller's frame -- the number of steps it accumulated before its last
	// clearFrameBuffer -- when no batch size was set: a frame that fits ONE pass has nothing to overlap that pass's launch tails and shade kernels with, two passes
	// hide each other's (measured on a 1/2 tile share of a 64-spp frame, where the automatic batch is the whole frame: 9.23 -> 8.49 ms per step; full frame and
	// 1/4, 1/8 shares unchanged).  Capacity is sized by effectiveBatch(), which this never exceeds.
	int lastFrameSteps = 0;
	int passSteps() const
	{
		int b = effectiveBatch();
		// under a sample mask the automatic size counts the active samples of a step, so that a thin mask does not make passes that are all launch tail;
		// bounded by what the slots were allocated for (effectiveBatch() steps of the whole frame).  Never smaller than without the mask: nActive <= ownedPixels
		if( batch == 0 && frame.masked && frame.nActive > 0 )
		{
			const uint64_t perStep = frame.nActive * MVRT_SPP_PER_STEP;
			uint64_t m = ( 66000000ull + perStep / 2 ) / perStep;
			const uint64_t fits = frame.ownedPixels * (uint64_t)b / frame.nActive;
			if( m > fits ) m = fits;
			if( m > MVRT_MAX_BATCH ) m = MVRT_MAX_BATCH;
			if( (int)m > b ) b = (int)m;
		}
		if( batch == 0 && lastFrameSteps >= 2 && b > ( lastFrameSteps + 1 ) / 2 ) b = ( lastFrameSteps + 1 ) / 2;
		return b;
	}
	// What allocWork budgets for, a policy and not a size: every in-flight pass owns ~190 bytes of path state per sample (two ping-pong path sets, ray directions, hit
	// records, per-sample radiance).  Feature buffers on: + 32 B of partial sums per pixel and merged step of every pass in flight, + the two accumulation buffers;
	// moments on: + their accumulation buffer (they have no per-pass state)
	uint64_t budgetedBytes() const
	{
		const uint64_t pathState = (uint64_t)depth * frame.ownedPixels * MVRT_SPP_PER_STEP * (uint64_t)effectiveBatch() * 200ull;
		const uint64_t withAovs = aovs ? pathState + (uint64_t)depth * frame.ownedPixels * (uint64_t)effectiveBatch() * 32ull + frame.ownedPixels * 32ull : pathState;
		return moments ? withAovs + frame.ownedPixels * 16ull : withAovs;
	}
	PtFrame passFrame( int iteration, int nSteps, int traceGridDiv ) const
	{
		PtFrame f;
		f.width = frame.width;
		f.height = frame.height;
		f.tileIndex = tileIndex;
		f.tileCount = tileCount;
		f.ownedPixels = frame.ownedPixels;
		f.validOwnedPixels = frame.activePixels(); // (under a sample mask the pass numbers its tasks over the active list)
		f.iteration = iteration;
		f.nSteps = nSteps;
		f.traceGridDiv = traceGridDiv;
		f.useHints = originHints ? 1 : 0;
		return f;
	}
	// make `user` stream wait for every step that was issued on the internal streams
	int join( hipStream_t user )
	{
		if( flush() ) return 1;
		if( pendingJoin && lastAccum ) MVRT_HIP( hipStreamWaitEvent( user, lastAccum, 0 ) );
		pendingJoin = false;
		return 0;
	}
	int drain() // host-side: everything the internal streams hold has finished
	{
		if( flush() ) return 1;
		// depth 1 runs on the caller's stream, which the caller may have destroyed since: wait for the event recorded behind the pass
		if( lastAccum ) MVRT_HIP( hipEventSynchronize( lastAccum ) );
		for( Slot& sl : slots )
			if( sl.stream ) MVRT_HIP( hipStreamSynchronize( sl.stream ) );
		pendingJoin = false;
		pendingStream = nullptr;
		return 0;
	}
	~mvrt_pt()
	{
		for( Slot& sl : slots )
		{
			if( sl.stream )
			{
				(void)hipStreamSynchronize( sl.stream );
				(void)hipStreamDestroy( sl.stream );
			}
			if( sl.accumDone ) (void)hipEventDestroy( sl.accumDone );
		}
		if( forkEv ) (void)hipEventDestroy( forkEv );
	}
};

int ptFlush( mvrt_pt* pt ) { return pt->flush(); }
int ptDrain( mvrt_pt* pt ) { return pt->drain(); }

MVRT_EXPORT int mvrt_pt_create( mvrt_pt** out )
{
	mvrt_pt* pt = new mvrt_pt();
	pt->intersector = new mvrt_svo();
	pt->intersector->owner = pt;
	*out = pt;
	return 0;
}
MVRT_EXPORT int mvrt_pt_destroy( mvrt_pt* pt )
{
	if( pt )
	{
		mvrt_svo_destroy( pt->intersector );
		delete pt;
	}
	return 0;
}
MVRT_EXPORT int mvrt_pt_setup( mvrt_pt* pt, void* stream )
{
	REQUIRE( pt, "null argument" );
	// PMJSampler::setup, pmjSampler.hpp:114-144
	std::vector<float> samples( (size_t)2 * MVRT_PMJ_LENGTH * MVRT_PMJ_NSEQ );
	PCG32 rng;
	rng.setup( 0, 2525 );
	for( int i = 0; i < MVRT_PMJ_NSEQ; i++ ) pmj02Sequence( MVRT_PMJ_LENGTH, samples.data() + (size_t)2 * MVRT_PMJ_LENGTH * i, rng );
	if( pt->pmj.alloc( samples.size() * 4 ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( pt->pmj.p, samples.data(), samples.size() * 4, hipMemcpyHostToDevice, (hipStream_t)stream ) );
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	int dev = 0;
	MVRT_HIP( hipGetDevice( &dev ) );
	hipDeviceProp_t p;
	MVRT_HIP( hipGetDeviceProperties( &p, dev ) );
	pt->numCUs = p.multiProcessorCount;
	pt->setupDone = true;
	return 0;
}

MVRT_EXPORT int mvrt_pt_download_pmj( mvrt_pt* pt, float* tableHost )
{
	REQUIRE( pt && pt->pmj.p && tableHost, "mvrt_pt_download_pmj: call mvrt_pt_setup first" );
	MVRT_HIP( hipMemcpy( tableHost, pt->pmj.p, pt->pmj.bytes, hipMemcpyDeviceToHost ) ); // (default stream: mvrt_pt_setup waited for its upload)
	return 0;
}

MVRT_EXPORT int mvrt_pt_set_tile( mvrt_pt* pt, int tileIndex, int tileCount )
{
	REQUIRE( pt && tileCount >= 1 && tileIndex >= 0 && tileIndex < tileCount, "bad tile %d of %d", tileIndex, tileCount );
	if( pt->drain() ) return 1;
	pt->tileIndex = tileIndex;
	pt->tileCount = tileCount;
	pt->forgetFrame(); // nothing of the old tiling is kept: the next resize allocates for the new one
	return 0;
}
MVRT_EXPORT uint64_t mvrt_pt_owned_pixels( const mvrt_pt* pt ) { return pt ? pt->frame.ownedPixels : 0; }

// Every array of a slot's PtBuffers in its one block, in a fixed order, each padded to 256 B so the float4 reads of Ls* stay aligned.  Returns the bytes taken;
// base == 0 only measures.  No kernel reads past the end of an array, so nothing is kept behind the last one.
static uint64_t carveWork( uintptr_t base, uint64_t cap, uint64_t nBlocks, PtBuffers& b )
{
	uint64_t off = 0;
	auto take = [&]( uint64_t bytes ) {
		void* r = (void*)( base + off );
		off += ( bytes + 255 ) & ~(uint64_t)255;
		return r;
	};
	for( int s = 0; s < 2; s++ )
	{
		PathSet& ps = b.set[s];
		ps.task = (uint32_t*)take( cap * 4 );
		ps.org = (uint32_t*)take( cap * 4 );
		float** f[] = { &ps.rox, &ps.roy, &ps.roz, &ps.rdx, &ps.rdy, &ps.rdz, &ps.Tx, &ps.Ty, &ps.Tz, &ps.Lx, &ps.Ly, &ps.Lz, &ps.nx, &ps.ny, &ps.nz };
		for( float** q : f ) *q = (float*)take( cap * 4 );
	}
	float** d[] = { &b.sx, &b.sy, &b.sz, &b.ex, &b.ey, &b.ez, &b.hitT, &b.Lsx, &b.Lsy, &b.Lsz };
	for( float** q : d ) *q = (float*)take( cap * 4 );
	b.hitPath = (uint64_t*)take( cap * 8 );
	b.hitEPath = (uint64_t*)take( cap * 8 );
	b.hitN = (uint8_t*)take( cap );
	b.hitS = (uint8_t*)take( cap );
	b.hitE = (uint8_t*)take( cap );
	b.blockCount = (uint32_t*)take( nBlocks * 4 );
	b.liveCount = (uint32_t*)take( 64 * 4 );
	b.cursors = (unsigned long long*)take( 16 * 8 );
	b.selfDev = (const PtBuffers*)take( sizeof( PtBuffers ) );
	b.tileBase = (uint32_t*)take( scanTileEntries( cap ) * 4 );
	return off;
}
int mvrt_pt::allocWorkSlot( Slot& sl )
{
	const uint64_t cap = frame.ownedPixels * MVRT_SPP_PER_STEP * effectiveBatch();
	const uint64_t nBlocks = scanCountEntries( cap ); // (padded: the scan reads whole 16-byte quads)
	PtBuffers measured;
	const uint64_t bytes = carveWork( 0, cap, nBlocks, measured );
	if( sl.work.alloc( bytes ) ) return 1;
	PtBuffers& b = sl.buf;
	REQUIRE( carveWork( (uintptr_t)sl.work.p, cap, nBlocks, b ) == bytes, "internal: the work block was measured as %llu bytes and carved differently", (unsigned long long)bytes );
	b.stats = statsBuf.as<unsigned long long>(); // shared by all slots (atomic tallies)
	b.cap = cap;
	// default stream: allocSlots drained every slot stream first, and the synchronous copy behind the memset on the same stream returns only after both
	MVRT_HIP( hipMemset( b.liveCount, 0, 64 * 4 ) );
	MVRT_HIP( hipMemcpy( (void*)b.selfDev, &b, sizeof( PtBuffers ), hipMemcpyHostToDevice ) );
	if( aovs && sl.aovPart.alloc( cap / MVRT_SPP_PER_STEP * 2 * sizeof( float4 ) ) ) return 1; // a block of its own: the sizes above are those of a library without feature buffers
	return 0;
}
int mvrt_pt::allocSlots()
{
	if( drain() ) return 1;
	if( !statsBuf.p )
	{
		if( statsBuf.alloc( 64 * 8 ) ) return 1;
		MVRT_HIP( hipMemset( statsBuf.p, 0, 64 * 8 ) ); // (default stream: completed by the synchronous copy of the first allocWorkSlot below, before any slot stream runs)
	}
	if( !forkEv ) MVRT_HIP( hipEventCreateWithFlags( &forkEv, hipEventDisableTiming ) );
	for( Slot& sl : slots ) sl.release(); // what is allocated now is about to be replaced: released first, allocated second
	// Footprint: depth x batch x ownedPixels x 16 x ~190 B (budgetedBytes), e.g. 3 x 2 x 6.3 GB at 1920x1080 (the reference: a fixed 1.24 GB stack slab).  It
	// must fit beside the octree: when it would take more than 70 % of the HBM that is free right now, merge fewer steps per pass first, then
	// keep fewer passes in flight.  Results do not depend on either.
	size_t freeB = 0, totalB = 0;
	MVRT_HIP( hipMemGetInfo( &freeB, &totalB ) );
	if( testFreeBytes ) freeB = (size_t)testFreeBytes; // mvrt_pt_set_test_free_bytes: pretend this much HBM is free (failure-path tests)
	batchCap = MVRT_MAX_BATCH;
	depth = depthWanted;
	const uint64_t budget = (uint64_t)( 0.7 * (double)freeB );
	while( budgetedBytes() > budget && effectiveBatch() > 1 ) batchCap = effectiveBatch() - 1;
	while( budgetedBytes() > budget && depth > 1 ) depth--;
	REQUIRE( budgetedBytes() <= budget, "frame of %llu owned pixels needs %.1f GB of path state, %.1f GB of HBM are free (split the frame into tiles: mvrt_pt_set_tile)",
			 (unsigned long long)frame.ownedPixels, budgetedBytes() / 1e9, freeB / 1e9 );
	for( int i = 0; i < 4; i++ )
	{
		Slot& sl = slots[i];
		if( i >= depth ) // no pass runs here: not its traversal workspace either
		{
			sl.trace = Workspace();
			continue;
		}
		if( allocWorkSlot( sl ) ) return 1;
		if( depth > 1 && !sl.stream )
		{
			// (experiment knob: slot streams of different priorities live in different hardware-queue pools and are dispatched in priority order)
			const int mode = (int)mvrtKnob( "MVRT_SLOT_PRIO", 0 );
			int lo = 0, hi = 0;
			MVRT_HIP( hipDeviceGetStreamPriorityRange( &lo, &hi ) );
			const int prio = mode == 0 ? 0 : ( mode == 1 ? ( i == 0 ? hi : ( i == 2 ? lo : 0 ) ) : ( i % 2 == 0 ? hi : lo ) );
			MVRT_HIP( hipStreamCreateWithPriority( &sl.stream, hipStreamNonBlocking, prio ) );
		}
		if( !sl.accumDone ) MVRT_HIP( hipEventCreateWithFlags( &sl.accumDone, hipEventDisableTiming ) );
	}
	nextSlot = lastSlot = 0;
	lastAccum = nullptr;
	return 0;
}
MVRT_EXPORT int mvrt_pt_clear_framebuffer( mvrt_pt* pt, void* stream )
{
	REQUIRE( pt && pt->frame.f32.p, "no frame buffer" );
	if( pt->join( (hipStream_t)stream ) ) return 1;
	if( pt->steps >= 2 ) pt->lastFrameSteps = pt->steps; // the caller's frame length (passSteps); a one-step frame says nothing about the next one
	pt->steps = 0; // PathTracer.hpp:100
	pt->frame.masked = false; // a new frame needs every pixel (the steps in flight still read the list: it is kept)
	return pt->frame.clear( (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_pt_resize_framebuffer_if_needed( mvrt_pt* pt, void* stream, int width, int height )
{
	REQUIRE( pt && width > 0 && height > 0, "bad resolution %dx%d", width, height );
	mvrt_pt::Frame& fr = pt->frame;
	if( fr.f32.p && fr.width == width && fr.height == height ) return 0;
	if( pt->drain() ) return 1;
	const uint64_t nPix = (uint64_t)width * height;
	const uint64_t nBlocks = ( nPix + MVRT_TILE_PIXELS - 1 ) / MVRT_TILE_PIXELS;
	// blocks b with b % tileCount == tileIndex
	const uint64_t myBlocks = nBlocks > (uint64_t)pt->tileIndex ? ( nBlocks - pt->tileIndex + pt->tileCount - 1 ) / pt->tileCount : 0;
	// every rank pads to the same count so an all-gather of equal chunks works
	const uint64_t maxBlocks = ( nBlocks + pt->tileCount - 1 ) / pt->tileCount;
	fr.ownedPixels = maxBlocks * MVRT_TILE_PIXELS;
	uint64_t valid = myBlocks * MVRT_TILE_PIXELS;
	if( myBlocks > 0 )
	{
		const uint64_t lastGlobalBlock = ( myBlocks - 1 ) * pt->tileCount + pt->tileIndex;
		const uint64_t endPix = ( lastGlobalBlock + 1 ) * MVRT_TILE_PIXELS;
		if( endPix > nPix ) valid -= endPix - nPix;
	}
	fr.validOwnedPixels = valid;
	fr.width = width;
	fr.height = height;
	fr.releaseDenoised(); // (a denoised image of the old size)
	fr.dropMask();		  // (a mask of the old size)
	if( fr.alloc( pt->aovs, pt->moments ) ) return pt->forgetFrame(); // (no frame without all of its buffers)
	if( pt->allocWork() ) return 1;
	return mvrt_pt_clear_framebuffer( pt, stream ); // :88
}

MVRT_EXPORT int mvrt_pt_load_hdri( mvrt_pt* pt, void* stream, const float* rgbaHost, int width, int height, const float* rgbaPrimaryHost, int widthPrimary,
								   int heightPrimary )
{
	REQUIRE( pt && rgbaHost && width > 0 && height > 0, "mvrt_pt_load_hdri: bad image" );
	// refused before a pointer is read or a byte allocated: the table kernels and the lookups index pixels with 32-bit integers
	REQUIRE( !rgbaPrimaryHost || ( widthPrimary > 0 && heightPrimary > 0 ), "mvrt_pt_load_hdri: bad primary image size %dx%d", widthPrimary, heightPrimary );
	REQUIRE( (uint64_t)width * height < ( 1ull << 31 ), "mvrt_pt_load_hdri: %dx%d is 2^31 pixels or more", width, height );
	REQUIRE( !rgbaPrimaryHost || (uint64_t)widthPrimary * heightPrimary < ( 1ull << 31 ), "mvrt_pt_load_hdri: primary %dx%d is 2^31 pixels or more", widthPrimary, heightPrimary );
	if( pt->drain() ) return 1;
	hipStream_t st = (hipStream_t)stream;
	const uint64_t n = (uint64_t)width * height;
	mvrt_pt::Hdri h; // built aside: a failure leaves the map that is loaded (or none) in place
	if( h.pixels.alloc( n * 16 ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( h.pixels.p, rgbaHost, n * 16, hipMemcpyHostToDevice, st ) );
	DevBuf satF64;
	if( satF64.alloc( ( n + 7 ) * 8 ) ) return 1; // the running table, then the seven totals
	// renderCommon.hpp:243-311: uniform table, then one cosine-weighted table per axis
	const f3 axes[6] = { mk3( 1, 0, 0 ), mk3( -1, 0, 0 ), mk3( 0, 1, 0 ), mk3( 0, -1, 0 ), mk3( 0, 0, 1 ), mk3( 0, 0, -1 ) };
	for( int i = 0; i < 7; i++ )
	{
		if( h.sat[i].alloc( n * 4 ) ) return 1;
		if( launchHdriSat( h.pixels.as<float4>(), width, height, satF64.as<double>(), h.sat[i].as<uint32_t>(), i > 0, i > 0 ? axes[i - 1] : mk3( 0, 0, 0 ), satF64.as<double>() + n + i, st ) )
			return 1;
	}
	h.dev.pixels = h.pixels.as<float4>();
	h.dev.sat = h.sat[0].as<uint32_t>();
	for( int i = 0; i < 6; i++ ) h.dev.sats[i] = h.sat[i + 1].as<uint32_t>();
	h.dev.width = h.dev.widthPrimary = width; // no primary map: see mvrt.h, the reference would index with 0x0 here
	h.dev.height = h.dev.heightPrimary = height;
	if( rgbaPrimaryHost ) // HDRI::loadPrimary, :315-326
	{
		const uint64_t np = (uint64_t)widthPrimary * heightPrimary;
		if( h.primary.alloc( np * 16 ) ) return 1;
		MVRT_HIP( hipMemcpyAsync( h.primary.p, rgbaPrimaryHost, np * 16, hipMemcpyHostToDevice, st ) );
		h.dev.pixelsPrimary = h.primary.as<float4>();
		h.dev.widthPrimary = widthPrimary;
		h.dev.heightPrimary = heightPrimary;
	}
	MVRT_HIP( hipStreamSynchronize( st ) ); // :313 (and satF64 is released on return)
	double totals[7];
	MVRT_HIP( hipMemcpy( totals, satF64.as<double>() + n, sizeof( totals ), hipMemcpyDeviceToHost ) ); // (default stream: behind the hipStreamSynchronize( st ) above)
	for( int i = 0; i < 7; i++ ) // a table without a total > 0 is all zeros and selects nothing (mvrt.h): the shade kernel tests this bit, not memory
		if( !( totals[i] > 0.0 ) ) h.dev.zeroTables |= 1u << i;
	h.dev.scale = pt->hdri.dev.scale;
	pt->hdri = std::move( h );
	return 0;
}
MVRT_EXPORT int mvrt_pt_load_hdri_file( mvrt_pt* pt, void* stream, const char* file, const char* filePrimary )
{
	std::vector<float> a, b;
	int w = 0, h = 0, wp = 0, hp = 0;
	if( loadRgbe( file, a, &w, &h ) ) return 1;
	if( filePrimary && loadRgbe( filePrimary, b, &wp, &hp ) ) return 1;
	return mvrt_pt_load_hdri( pt, stream, a.data(), w, h, filePrimary ? b.data() : nullptr, wp, hp );
}
// host-only: the decoder behind mvrt_pt_load_hdri_file (pr::Image2DRGBA32::loadFromHDR's role, PathTracer.hpp:106-113)
MVRT_EXPORT int mvrt_rgbe_read_file( const char* file, float* rgbaHost, uint64_t capacityPixels, int* width, int* height )
{
	REQUIRE( file && width && height, "null argument" );
	std::vector<float> a;
	if( loadRgbe( file, a, width, height ) ) return 1;
	if( !rgbaHost ) return 0;
	REQUIRE( (uint64_t)*width * *height <= capacityPixels, "%s: %dx%d pixels do not fit %llu", file, *width, *height, (unsigned long long)capacityPixels );
	memcpy( rgbaHost, a.data(), a.size() * sizeof( float ) );
	return 0;
}
MVRT_EXPORT int mvrt_pt_download_hdri_sat( mvrt_pt* pt, int which, uint32_t* satHost )
{
	REQUIRE( pt && which >= 0 && which < 7 && pt->hdri.sat[which].p, "no such HDRI table" );
	MVRT_HIP( hipMemcpy( satHost, pt->hdri.sat[which].p, pt->hdri.sat[which].bytes, hipMemcpyDeviceToHost ) ); // (default stream: mvrt_pt_load_hdri waited for its tables)
	return 0;
}
MVRT_EXPORT int mvrt_pt_set_hdri_scale( mvrt_pt* pt, float scale )
{
	REQUIRE( pt, "null argument" );
	if( pt->flush() ) return 1; // pending steps are launched with the scale they were issued under (HDRI is a by-value kernel argument)
	pt->hdri.dev.scale = scale;
	return 0;
}
MVRT_EXPORT int mvrt_pt_update_scene( mvrt_pt* pt, const float* verticesHost, const float* vcolorsHost, const float* vemissionsHost, uint64_t nVertices, void* stream,
									  const float origin[3], float dps, int gridRes )
{
	REQUIRE( pt, "null argument" );
	if( pt->drain() ) return 1;
	return mvrt_svo_build( pt->intersector, verticesHost, vcolorsHost, vemissionsHost, nVertices, stream, origin, dps, gridRes );
}
MVRT_EXPORT mvrt_svo* mvrt_pt_intersector( mvrt_pt* pt ) { return pt ? pt->intersector : nullptr; }

MVRT_EXPORT int mvrt_pt_step( mvrt_pt* pt, void* stream, const float camera[15] )
{
	REQUIRE( pt && pt->setupDone, "mvrt_pt_step: call mvrt_pt_setup first" );
	REQUIRE( !pt->intersector->empty(), "mvrt_pt_step: no scene (updateScene / upload first)" );
	REQUIRE( pt->frame.f32.p, "mvrt_pt_step: no frame buffer (resizeFrameBufferIfNeeded first)" );
	REQUIRE( !( 0.0f < pt->hdri.dev.scale ) || pt->hdri.dev.pixels, "mvrt_pt_step: HDRI enabled (scale > 0) but none loaded" );
	// deferred: remember the camera; the pass is launched when `batch` steps are pending or a consumer joins
	if( !pt->pendingCams.empty() && pt->pendingStream != (hipStream_t)stream && pt->flush() ) return 1; // (steps of another stream go first)
	if( pt->pendingCams.empty() ) // start a new pending run
	{
		pt->pendingIteration = pt->steps;
		pt->pendingStream = (hipStream_t)stream;
	}
	pt->steps++; // PathTracer.hpp:159
	if( pt->frame.masked && pt->frame.nActive == 0 ) return 0; // no pixel is active: the iteration is spent, nothing is launched
	pt->pendingCams.push_back( cameraFrom15( camera ) );
	if( (int)pt->pendingCams.size() >= pt->passSteps() ) return pt->flush( true ); // a full batch: the caller is still stepping
	return 0;
}
int mvrt_pt::flush( bool moreStepsFollow )
{
	if( pendingCams.empty() ) return 0;
	const int n = (int)pendingCams.size();
	// A SMALL pass (a tile share of a multi-GPU frame, a small frame) is dominated by the latency floors of its nine traversal
	// launches and by its un-overlapped shade kernels.  Two sibling passes on two streams, each traversal launch restricted to half
	// of the wave slots, overlap one pass's tails and shading with the other's traversal.  Same per-sample results; the frame-buffer
	// additions stay in step order through the event chain.
	const uint64_t samples = ( frame.masked ? frame.nActive : frame.ownedPixels ) * MVRT_SPP_PER_STEP * (uint64_t)n;
	static const uint64_t splitMax = (uint64_t)mvrtKnob( "MVRT_SPLIT_SMALL_MAX", 40000000ll );
	// ... but only when this pass would otherwise run ALONE: if the caller keeps stepping, or an earlier pass is still in flight, the
	// passes already overlap each other and halving their grids only slows them (measured: 2.68 -> 2.99 ms per step at 16 steps)
	const bool alone = !moreStepsFollow && ( !lastAccum || !pendingJoin || hipEventQuery( lastAccum ) == hipSuccess );
	const bool split = splitSmallPasses && alone && depth >= 2 && n >= 2 && samples <= splitMax;
	const std::vector<CameraPinhole> cams = std::move( pendingCams );
	pendingCams.clear();
	const int first = pendingIteration;
	if( !split ) return launchPass( cams.data(), first, n, 1 );
	// `ways` sibling passes (at most one per work-buffer slot and per step), each restricted to 1/ways of the wave slots
	static const int envWays = (int)mvrtKnob( "MVRT_SPLIT_WAYS", 2 );
	int ways = envWays < 2 ? 2 : envWays;
	if( ways > depth ) ways = depth;
	if( ways > n ) ways = n;
	int done = 0;
	for( int k = 0; k < ways; k++ )
	{
		const int cnt = ( n - done ) / ( ways - k );
		// (r02: each sibling's traversal launches took 1 / ways of the wave slots; r03 re-measured with the cheaper-to-drain kernel: full grids are 1-2 %
		//  better on a 1/8 share -- dragon 2.744 -> 2.698, rtcamp 2.421 -> 2.393 ms per step -- the dispatcher hands the slots of retiring waves to the sibling)
		static const int siblingDiv = (int)mvrtKnob( "MVRT_SIBLING_GRID_DIV", 1 );
		if( launchPass( cams.data() + done, first + done, cnt, siblingDiv > 0 ? siblingDiv : ways ) ) return 1;
		done += cnt;
	}
	return 0;
}
int mvrt_pt::launchPass( const CameraPinhole* cams, int iteration, int nSteps, int traceGridDiv )
{
	hipStream_t user = pendingStream;
	Slot& sl = slots[nextSlot];
	lastSlot = nextSlot;
	nextSlot = ( nextSlot + 1 ) % depth;
	REQUIRE( sl.buf.cap >= frame.activePixels() * MVRT_SPP_PER_STEP * nSteps, "internal: work buffers not allocated" );
	if( sl.trace.ensure( intersector->oct.info.levels, 0 ) ) return 1;
	sl.buf.dbgTasks = nullptr;
	if( debugCapture )
	{
		if( sl.dbg.bytes < sl.buf.cap * 4 * MVRT_MAX_DEPTH && sl.dbg.alloc( sl.buf.cap * 4 * MVRT_MAX_DEPTH ) ) return 1;
		sl.buf.dbgTasks = sl.dbg.as<uint32_t>();
	}
	hipStream_t run = user;
	hipEvent_t after = nullptr;
	if( depth > 1 )
	{
		run = sl.stream;
		MVRT_HIP( hipEventRecord( forkEv, user ) ); // everything the caller queued so far (clear, upload, ...) comes first
		MVRT_HIP( hipStreamWaitEvent( run, forkEv, 0 ) );
		after = lastAccum;
	}
	AovBuffers aov = { nullptr, nullptr, nullptr, nullptr };
	if( aovs )
	{
		REQUIRE( sl.aovPart.p && frame.albedo.p && frame.normalDepth.p, "internal: feature buffers not allocated" );
		aov.partA = sl.aovPart.as<float4>();
		aov.partN = aov.partA + sl.buf.cap / MVRT_SPP_PER_STEP;
		aov.albedo = frame.albedo.as<float4>();
		aov.normalDepth = frame.normalDepth.as<float4>();
	}
	REQUIRE( !moments || frame.moments.p, "internal: moments buffer not allocated" );
	int rc = launchPtStep( intersector->dev(), sl.trace.ws, hdri.dev, pmj.as<float2>(), cams, passFrame( iteration, nSteps, traceGridDiv ), sl.buf, frame.f32.as<float4>(), numCUs,
						   profiling ? &prof : nullptr, run, after, aovs ? &aov : nullptr, moments ? frame.moments.as<float4>() : nullptr, frame.passList() );
	if( rc ) return rc;
	MVRT_HIP( hipEventRecord( sl.accumDone, run ) );
	lastAccum = sl.accumDone;
	if( depth > 1 ) pendingJoin = true;
	return 0; // profiling events are collected lazily by mvrt_pt_get_stats (no sync inside step)
}
MVRT_EXPORT int mvrt_pt_step_matrices( mvrt_pt* pt, void* stream, const float view[16], const float proj[16], float focus, float lensR )
{
	float cam[15];
	mvrt_camera_from_matrices( view, proj, focus, lensR, cam );
	return mvrt_pt_step( pt, stream, cam );
}
MVRT_EXPORT int mvrt_pt_resolve( mvrt_pt* pt, void* stream )
{
	REQUIRE( pt && pt->frame.f32.p, "no frame buffer" );
	if( pt->join( (hipStream_t)stream ) ) return 1;
	return launchResolve( pt->frame.f32.as<float4>(), pt->frame.validOwnedPixels, pt->frame.u8.as<uchar4>(), (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_pt_to_image_async( mvrt_pt* pt, void* stream, uint8_t* rgbaHost )
{
	if( mvrt_pt_resolve( pt, stream ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( rgbaHost, pt->frame.u8.p, pt->frame.validOwnedPixels * 4, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
	return 0;
}
MVRT_EXPORT int mvrt_pt_get_steps( const mvrt_pt* pt ) { return pt ? pt->steps : 0; }
MVRT_EXPORT uint64_t mvrt_pt_get_number_of_voxels( const mvrt_pt* pt ) { return pt ? pt->intersector->oct.nVoxels : 0; }
MVRT_EXPORT uint64_t mvrt_pt_get_octree_bytes( const mvrt_pt* pt ) { return pt ? (uint64_t)pt->intersector->oct.nNodes * 68 : 0; }

// The blocking host copy of a buffer of the frame.  joined: the accumulation buffers, which the steps in flight still add to; the denoised image is read on
// the stream its denoise ran on
static int readBack( mvrt_pt* pt, const DevBuf& b, uint64_t bytes, bool joined, void* stream, float* rgbaHost )
{
	if( joined && pt->join( (hipStream_t)stream ) ) return 1;
	MVRT_HIP( hipMemcpyAsync( rgbaHost, b.p, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	return 0;
}
MVRT_EXPORT int mvrt_pt_read_framebuffer( mvrt_pt* pt, void* stream, float* rgbaHost )
{
	REQUIRE( pt && pt->frame.f32.p, "no frame buffer" );
	return readBack( pt, pt->frame.f32, pt->frame.accumBytes(), true, stream, rgbaHost );
}
MVRT_EXPORT float* mvrt_pt_framebuffer_dev( mvrt_pt* pt ) { return pt ? pt->frame.f32.as<float>() : nullptr; }

// ---- the optional accumulation buffers: first-hit feature buffers and luminance moments ---------------------------------------------------------
// One switch: `bufs` are the option's buffers in the frame, `goWithThem` what else of the frame is released when it is switched off, `what` its name in the
// messages.  Without a frame only the flag changes.  With one, switching on
// allocates and clears the buffers beside it -- a failure up to there releases what was just allocated and leaves the frame as it was, with the option off --
// and either direction ends in allocWork, since the option counts against the budget of the path state: a failure there leaves NO frame, like every reallocation.
static int allocCleared( std::initializer_list<DevBuf*> bufs, uint64_t bytes, const char* who, const char* what )
{
	for( DevBuf* b : bufs )
		if( b->alloc( bytes ) ) return 1;
	hipError_t e = hipSuccess;
	for( DevBuf* b : bufs )
		if( e == hipSuccess ) e = hipMemset( b->p, 0, bytes ); // (default stream: setOption drained the slot streams; waited for by the hipStreamSynchronize( nullptr ) below)
	if( e == hipSuccess ) e = hipStreamSynchronize( nullptr );
	if( e == hipSuccess ) return 0;
	mvrtSetError( "%s: clearing the %s failed: %s", who, what, hipGetErrorString( e ) );
	return 1;
}
int mvrt_pt::setOption( bool& flag, bool on, std::initializer_list<DevBuf*> bufs, std::initializer_list<DevBuf*> goWithThem, const char* who, const char* what )
{
	if( drain() ) return 1;
	if( on == flag ) return 0;
	REQUIRE( steps == 0, "%s: %d steps are accumulated in the frame buffer, the %s would not match its sample count (mvrt_pt_clear_framebuffer first)", who, steps, what );
	const bool failed = on && frame.f32.p && allocCleared( bufs, frame.accumBytes(), who, what );
	if( !on || failed )
		for( DevBuf* b : bufs ) b->release(); // (off means no buffer held)
	if( failed ) return 1;
	if( !on )
		for( DevBuf* b : goWithThem ) b->release();
	flag = on;
	return frame.f32.p ? allocWork() : 0;
}
MVRT_EXPORT int mvrt_pt_set_aovs( mvrt_pt* pt, int enable )
{
	REQUIRE( pt, "null argument" );
	return pt->setOption( pt->aovs, enable != 0, { &pt->frame.albedo, &pt->frame.normalDepth }, {}, "mvrt_pt_set_aovs", "feature buffers" );
}
MVRT_EXPORT int mvrt_pt_set_moments( mvrt_pt* pt, int enable )
{
	REQUIRE( pt, "mvrt_pt_set_moments: null argument" );
	// (switched off, the denoised image goes with the moments it was made from)
	return pt->setOption( pt->moments, enable != 0, { &pt->frame.moments }, { &pt->frame.denoised, &pt->frame.denoiseScratch }, "mvrt_pt_set_moments", "moments" );
}
// One lookup: the buffer of an option that is on and has a frame, or null and the reason
static DevBuf* optionBuffer( mvrt_pt* pt, bool ofMoments, int which, const char* who )
{
	if( !pt )
	{
		mvrtSetError( "%s: null argument", who );
		return nullptr;
	}
	if( !ofMoments && which != MVRT_AOV_ALBEDO && which != MVRT_AOV_NORMAL_DEPTH )
	{
		mvrtSetError( "%s: no feature buffer %d (MVRT_AOV_ALBEDO, MVRT_AOV_NORMAL_DEPTH)", who, which );
		return nullptr;
	}
	const bool on = ofMoments ? pt->moments : pt->aovs;
	DevBuf* b = ofMoments ? &pt->frame.moments : ( which == MVRT_AOV_ALBEDO ? &pt->frame.albedo : &pt->frame.normalDepth );
	if( on && b->p ) return b;
	mvrtSetError( on ? "%s: no frame buffer" : ( ofMoments ? "%s: the moments are off (mvrt_pt_set_moments)" : "%s: feature buffers are off (mvrt_pt_set_aovs)" ), who );
	return nullptr;
}
MVRT_EXPORT float* mvrt_pt_aov_dev( mvrt_pt* pt, int which )
{
	DevBuf* b = optionBuffer( pt, false, which, "mvrt_pt_aov_dev" );
	return b ? b->as<float>() : nullptr;
}
MVRT_EXPORT int mvrt_pt_read_aov( mvrt_pt* pt, void* stream, int which, float* rgbaHost )
{
	DevBuf* b = optionBuffer( pt, false, which, "mvrt_pt_read_aov" );
	if( !b ) return 1;
	REQUIRE( rgbaHost, "mvrt_pt_read_aov: null argument" );
	return readBack( pt, *b, pt->frame.accumBytes(), true, stream, rgbaHost );
}
MVRT_EXPORT float* mvrt_pt_moments_dev( mvrt_pt* pt )
{
	DevBuf* b = optionBuffer( pt, true, 0, "mvrt_pt_moments_dev" );
	return b ? b->as<float>() : nullptr;
}
MVRT_EXPORT int mvrt_pt_read_moments( mvrt_pt* pt, void* stream, float* rgbaHost )
{
	DevBuf* b = optionBuffer( pt, true, 0, "mvrt_pt_read_moments" );
	if( !b ) return 1;
	REQUIRE( rgbaHost, "mvrt_pt_read_moments: null argument" );
	return readBack( pt, *b, pt->frame.accumBytes(), true, stream, rgbaHost );
}

// ---- denoiser ---------------------------------------------------------------------------------------------------
MVRT_EXPORT int mvrt_denoise_default_params( mvrt_denoise_params* p )
{
	REQUIRE( p, "mvrt_denoise_default_params: null argument" );
	memset( p, 0, sizeof( *p ) );
	p->structBytes = (uint32_t)sizeof( mvrt_denoise_params );
	p->iterations = 5;
	p->sigmaNormal = 0.5f;
	p->sigmaDepth = 0.05f;
	p->sigmaCoverage = 0.25f;
	p->sigmaLuminance = 2.0f;
	p->albedoFloor = 0.01f;
	return 0;
}
// every rule on the parameters, on the host; in == NULL: the defaults
static int denoiseParams( const mvrt_denoise_params* in, mvrt_denoise_params* out, const char* who )
{
	mvrt_denoise_default_params( out );
	if( !in ) return 0;
	REQUIRE( in->structBytes == sizeof( mvrt_denoise_params ), "%s: params->structBytes is %u, sizeof( mvrt_denoise_params ) is %u (mvrt_denoise_default_params fills it)", who, in->structBytes,
			 (unsigned)sizeof( mvrt_denoise_params ) );
	REQUIRE( in->iterations >= 1 && in->iterations <= 8, "%s: iterations %d outside 1..8", who, in->iterations );
	REQUIRE( in->sigmaNormal > 0.0f, "%s: sigmaNormal %g is not greater than 0", who, (double)in->sigmaNormal );
	REQUIRE( in->sigmaDepth > 0.0f, "%s: sigmaDepth %g is not greater than 0", who, (double)in->sigmaDepth );
	REQUIRE( in->sigmaCoverage > 0.0f, "%s: sigmaCoverage %g is not greater than 0", who, (double)in->sigmaCoverage );
	REQUIRE( in->sigmaLuminance > 0.0f, "%s: sigmaLuminance %g is not greater than 0", who, (double)in->sigmaLuminance );
	REQUIRE( in->albedoFloor > 0.0f, "%s: albedoFloor %g is not greater than 0", who, (double)in->albedoFloor );
	// +inf passes the rules above, and sigmaLuminance * sqrt( 0 ) = inf * 0 = NaN turns the whole frame NaN by the contract's own arithmetic
	REQUIRE( in->sigmaNormal - in->sigmaNormal == 0.0f, "%s: sigmaNormal %g is not finite", who, (double)in->sigmaNormal );
	REQUIRE( in->sigmaDepth - in->sigmaDepth == 0.0f, "%s: sigmaDepth %g is not finite", who, (double)in->sigmaDepth );
	REQUIRE( in->sigmaCoverage - in->sigmaCoverage == 0.0f, "%s: sigmaCoverage %g is not finite", who, (double)in->sigmaCoverage );
	REQUIRE( in->sigmaLuminance - in->sigmaLuminance == 0.0f, "%s: sigmaLuminance %g is not finite", who, (double)in->sigmaLuminance );
	REQUIRE( in->albedoFloor - in->albedoFloor == 0.0f, "%s: albedoFloor %g is not finite", who, (double)in->albedoFloor );
	REQUIRE( in->sigmaNormal * in->sigmaNormal > 0.0f, "%s: sigmaNormal %g is too small, its square is not greater than 0 (the centre tap would be 0 / 0)", who, (double)in->sigmaNormal );
	REQUIRE( ( in->flags & ~(uint32_t)MVRT_DENOISE_NO_DEMODULATION ) == 0, "%s: unknown flags 0x%x", who, in->flags );
	*out = *in;
	return 0;
}
static bool denoiseSizeOk( int width, int height ) { return width > 0 && height > 0 && (uint64_t)width * (uint64_t)height <= 0x7FFFFFFFull; } // (32-bit pixel indices)
MVRT_EXPORT uint64_t mvrt_denoise_scratch_bytes( int width, int height )
{
	if( !denoiseSizeOk( width, height ) )
	{
		mvrtSetError( "mvrt_denoise_scratch_bytes: bad resolution %dx%d (width and height must be greater than 0)", width, height );
		return 0;
	}
	return denoiseScratchBytes( (uint64_t)width * height );
}
MVRT_EXPORT int mvrt_denoise_buffers( const float* colorDev, const float* albedoDev, const float* normalDepthDev, const float* momentsDev, int width, int height,
									  const mvrt_denoise_params* params, float* outDev, void* scratchDev, uint64_t scratchBytes, void* stream )
{
	REQUIRE( denoiseSizeOk( width, height ), "mvrt_denoise_buffers: bad resolution %dx%d (width and height must be greater than 0)", width, height );
	mvrt_denoise_params P;
	if( denoiseParams( params, &P, "mvrt_denoise_buffers" ) ) return 1;
	REQUIRE( colorDev && albedoDev && normalDepthDev && momentsDev && outDev && scratchDev, "mvrt_denoise_buffers: null argument" );
	const uint64_t need = denoiseScratchBytes( (uint64_t)width * height );
	REQUIRE( scratchBytes >= need, "mvrt_denoise_buffers: scratch too small, %llu bytes given, a %dx%d frame needs %llu (mvrt_denoise_scratch_bytes)", (unsigned long long)scratchBytes, width,
			 height, (unsigned long long)need );
	return launchDenoise( (const float4*)colorDev, (const float4*)albedoDev, (const float4*)normalDepthDev, (const float4*)momentsDev, width, height, P, (float4*)outDev, scratchDev,
						  (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_pt_denoise( mvrt_pt* pt, void* stream, const mvrt_denoise_params* params )
{
	REQUIRE( pt, "mvrt_pt_denoise: null argument" );
	mvrt_denoise_params P;
	if( denoiseParams( params, &P, "mvrt_pt_denoise" ) ) return 1;
	REQUIRE( pt->tileCount == 1, "mvrt_pt_denoise: this handle renders tile %d of %d; the filter needs the whole frame -- assemble the buffers (mvrt_pt_assemble_tiles) and call mvrt_denoise_buffers",
			 pt->tileIndex, pt->tileCount );
	REQUIRE( pt->aovs, "mvrt_pt_denoise: the feature buffers are off (mvrt_pt_set_aovs)" );
	REQUIRE( pt->moments, "mvrt_pt_denoise: the moments are off (mvrt_pt_set_moments)" );
	REQUIRE( pt->steps > 0, "mvrt_pt_denoise: no steps yet (the frame buffer holds no sample)" );
	mvrt_pt::Frame& fr = pt->frame;
	REQUIRE( fr.f32.p && fr.albedo.p && fr.normalDepth.p && fr.moments.p, "mvrt_pt_denoise: no frame buffer" );
	if( pt->join( (hipStream_t)stream ) ) return 1;
	const uint64_t nPix = (uint64_t)fr.width * fr.height;
	const uint64_t scratch = denoiseScratchBytes( nPix );
	const bool kept = fr.denoised.p && fr.denoised.bytes == nPix * sizeof( float4 ) && fr.denoiseScratch.bytes == scratch;
	// nothing of the frame is touched: a failure leaves it, the steps and the feature buffers as they are, and no denoised buffer
	if( ( !kept && ( fr.denoised.alloc( nPix * sizeof( float4 ) ) || fr.denoiseScratch.alloc( scratch ) ) ) ||
		launchDenoise( fr.f32.as<float4>(), fr.albedo.as<float4>(), fr.normalDepth.as<float4>(), fr.moments.as<float4>(), fr.width, fr.height, P, fr.denoised.as<float4>(), fr.denoiseScratch.p,
					   (hipStream_t)stream ) )
	{
		fr.releaseDenoised();
		return 1;
	}
	return 0;
}
// ---- adaptive sampling: the sample mask and the error mask ----------------------------------------------------------------------------------------
MVRT_EXPORT int mvrt_pt_set_sample_mask( mvrt_pt* pt, void* stream, const uint8_t* maskDev, uint64_t* nActiveOut )
{
	REQUIRE( pt, "mvrt_pt_set_sample_mask: null argument" );
	mvrt_pt::Frame& fr = pt->frame;
	REQUIRE( fr.f32.p, "mvrt_pt_set_sample_mask: no frame buffer" );
	if( pt->flush() ) return 1; // the pending steps run under the mask they were issued under
	if( !maskDev )
	{
		fr.masked = false;
		if( nActiveOut ) *nActiveOut = fr.validOwnedPixels;
		return 0;
	}
	// built aside: a failure leaves the mask that is in force (or none) in force, and the steps in flight go on reading the list they were launched with
	const uint64_t n = fr.validOwnedPixels;
	DevBuf list, scratch;
	const uint64_t rankBytes = ( n * 4 + 255 ) & ~(uint64_t)255, blockBytes = ( ( scanCountEntries( n ) + scanTileEntries( n ) ) * 4 + 255 ) & ~(uint64_t)255; // (counts, then tile sums)
	if( list.alloc( fr.ownedPixels * 4 ) || scratch.alloc( rankBytes + blockBytes + 4 ) ) return 1;
	uint32_t* kept = (uint32_t*)( scratch.as<uint8_t>() + rankBytes + blockBytes );
	uint32_t count = 0;
	if( n ) // (a rank of a tile split may own nothing)
	{
		if( launchActiveList( maskDev, n, list.as<uint32_t>(), kept, scratch.as<uint32_t>(), (uint32_t*)( scratch.as<uint8_t>() + rankBytes ), (hipStream_t)stream ) ) return 1;
		MVRT_HIP( hipMemcpyAsync( &count, kept, 4, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
		MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) ); // launch sizes need the count, and the caller's array is free again
	}
	if( pt->drain() ) return 1; // the list in force is replaced: nothing reads it any more
	if( count == n ) // every valid pixel is active, which IS no mask: the steps take the unmasked kernels, without the lookups through a list that says slot == pixel
	{
		fr.dropMask();
		if( nActiveOut ) *nActiveOut = count;
		return 0;
	}
	fr.activeList = std::move( list );
	fr.nActive = count;
	fr.masked = true;
	if( nActiveOut ) *nActiveOut = count;
	return 0;
}
MVRT_EXPORT uint64_t mvrt_pt_active_pixels( const mvrt_pt* pt ) { return pt && pt->frame.f32.p ? pt->frame.activePixels() : 0; }
MVRT_EXPORT int mvrt_pt_error_mask( mvrt_pt* pt, void* stream, float threshold, float lumFloor, int minSamples, int maxSamples, uint8_t* maskDev, uint64_t* nActiveOut )
{
	REQUIRE( pt && maskDev, "mvrt_pt_error_mask: null argument" );
	REQUIRE( threshold > 0.0f, "mvrt_pt_error_mask: threshold %g is not greater than 0", (double)threshold );
	REQUIRE( lumFloor > 0.0f, "mvrt_pt_error_mask: lumFloor %g is not greater than 0", (double)lumFloor );
	REQUIRE( minSamples >= 1, "mvrt_pt_error_mask: minSamples %d is less than 1", minSamples );
	REQUIRE( maxSamples >= 0, "mvrt_pt_error_mask: maxSamples %d is negative (0 = no limit)", maxSamples );
	REQUIRE( pt->moments, "mvrt_pt_error_mask: the moments are off (mvrt_pt_set_moments)" );
	mvrt_pt::Frame& fr = pt->frame;
	REQUIRE( fr.f32.p && fr.moments.p, "mvrt_pt_error_mask: no frame buffer" );
	if( pt->join( (hipStream_t)stream ) ) return 1;
	if( !fr.errorCount.p && fr.errorCount.alloc( 4 ) ) return 1;
	if( launchErrorMask( fr.f32.as<float4>(), fr.moments.as<float4>(), fr.validOwnedPixels, fr.ownedPixels, threshold, lumFloor, minSamples, maxSamples, maskDev,
						 fr.errorCount.as<uint32_t>(), (hipStream_t)stream ) )
		return 1;
	uint32_t count = 0;
	MVRT_HIP( hipMemcpyAsync( &count, fr.errorCount.p, 4, hipMemcpyDeviceToHost, (hipStream_t)stream ) );
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	if( nActiveOut ) *nActiveOut = count;
	return 0;
}

MVRT_EXPORT float* mvrt_pt_denoised_dev( mvrt_pt* pt ) { return pt ? pt->frame.denoised.as<float>() : nullptr; }
MVRT_EXPORT int mvrt_pt_read_denoised( mvrt_pt* pt, void* stream, float* rgbaHost )
{
	REQUIRE( pt && rgbaHost, "mvrt_pt_read_denoised: null argument" );
	REQUIRE( pt->frame.denoised.p, "mvrt_pt_read_denoised: no denoised buffer (mvrt_pt_denoise first)" );
	return readBack( pt, pt->frame.denoised, (uint64_t)pt->frame.width * pt->frame.height * 16, false, stream, rgbaHost );
}
MVRT_EXPORT uint8_t* mvrt_pt_framebuffer_u8_dev( mvrt_pt* pt ) { return pt ? pt->frame.u8.as<uint8_t>() : nullptr; }
MVRT_EXPORT const float* mvrt_pt_sample_radiance_dev( mvrt_pt* pt )
{
	if( !pt ) return nullptr;
	(void)pt->drain();
	return pt->slots[pt->lastSlot].buf.Lsx;
}
MVRT_EXPORT int mvrt_pt_read_sample_radiance( mvrt_pt* pt, float* xyzHost, uint64_t nSamples )
{
	REQUIRE( pt && xyzHost, "null argument" );
	if( pt->drain() ) return 1;
	const PtBuffers& b = pt->slots[pt->lastSlot].buf;
	REQUIRE( b.Lsx && nSamples <= b.cap, "no such samples" );
	MVRT_HIP( hipMemcpy( xyzHost, b.Lsx, nSamples * 4, hipMemcpyDeviceToHost ) ); // (default stream, the three copies: behind the drain above)
	MVRT_HIP( hipMemcpy( xyzHost + nSamples, b.Lsy, nSamples * 4, hipMemcpyDeviceToHost ) );
	MVRT_HIP( hipMemcpy( xyzHost + 2 * nSamples, b.Lsz, nSamples * 4, hipMemcpyDeviceToHost ) );
	return 0;
}
MVRT_EXPORT int mvrt_pt_join( mvrt_pt* pt, void* stream )
{
	REQUIRE( pt, "null argument" );
	return pt->join( (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_pt_set_batch_steps( mvrt_pt* pt, int maxSteps )
{
	REQUIRE( pt && maxSteps >= 0 && maxSteps <= MVRT_MAX_BATCH, "batch must be 0 (automatic) or 1..%d", MVRT_MAX_BATCH );
	if( pt->drain() ) return 1;
	pt->batch = maxSteps;
	if( pt->frame.f32.p ) return pt->allocWork();
	return 0;
}
MVRT_EXPORT int mvrt_pt_set_split_small_passes( mvrt_pt* pt, int enable )
{
	REQUIRE( pt, "null argument" );
	if( pt->drain() ) return 1;
	pt->splitSmallPasses = enable != 0;
	return 0;
}
MVRT_EXPORT int mvrt_pt_set_origin_hints( mvrt_pt* pt, int enable )
{
	REQUIRE( pt, "null argument" );
	if( pt->flush() ) return 1;
	pt->originHints = enable != 0;
	return 0;
}
MVRT_EXPORT int mvrt_pt_set_pipeline_depth( mvrt_pt* pt, int depth )
{
	REQUIRE( pt && depth >= 1 && depth <= 4, "pipeline depth must be 1..4" );
	if( pt->drain() ) return 1;
	pt->depth = pt->depthWanted = depth;
	if( pt->frame.f32.p ) return pt->allocWork();
	return 0;
}

MVRT_EXPORT int mvrt_pt_assemble_tiles( const float* gatheredDev, int tileCount, uint64_t rankStridePixels, int width, int height, float* frameDev, void* stream )
{
	REQUIRE( gatheredDev && frameDev && tileCount >= 1, "bad arguments" );
	return launchAssembleTiles( (const float4*)gatheredDev, tileCount, rankStridePixels, width, height, (float4*)frameDev, (hipStream_t)stream );
}
MVRT_EXPORT int mvrt_resolve_buffer( const float* rgbaF32Dev, uint64_t nPixels, uint8_t* rgbaU8Dev, void* stream )
{
	return launchResolve( (const float4*)rgbaF32Dev, nPixels, (uchar4*)rgbaU8Dev, (hipStream_t)stream );
}

MVRT_EXPORT int mvrt_pt_set_debug_capture( mvrt_pt* pt, int enabled )
{
	REQUIRE( pt, "null argument" );
	if( pt->drain() ) return 1;
	pt->debugCapture = enabled != 0;
	if( !enabled )
		for( mvrt_pt::Slot& sl : pt->slots ) sl.dbg.release();
	return 0;
}
MVRT_EXPORT int mvrt_pt_read_debug_stage( mvrt_pt* pt, int stage, uint32_t* tasksHost, uint64_t capacity, uint32_t* survivorsOut )
{
	REQUIRE( pt && stage >= 0 && stage < MVRT_MAX_DEPTH && survivorsOut, "bad arguments" );
	if( pt->drain() ) return 1;
	const mvrt_pt::Slot& sl = pt->slots[pt->lastSlot];
	REQUIRE( sl.buf.dbgTasks, "debug capture was not enabled for the last pass" );
	MVRT_HIP( hipMemcpy( survivorsOut, sl.buf.liveCount + stage + 1, 4, hipMemcpyDeviceToHost ) ); // (default stream, both copies: behind the drain above)
	REQUIRE( *survivorsOut <= capacity && *survivorsOut <= sl.buf.cap, "tasksHost holds %llu entries, stage %d kept %u", (unsigned long long)capacity, stage, *survivorsOut );
	if( tasksHost && *survivorsOut ) MVRT_HIP( hipMemcpy( tasksHost, sl.buf.dbgTasks + (uint64_t)stage * sl.buf.cap, (uint64_t)*survivorsOut * 4, hipMemcpyDeviceToHost ) );
	return 0;
}

MVRT_EXPORT int mvrt_pt_set_test_free_bytes( mvrt_pt* pt, uint64_t bytes )
{
	REQUIRE( pt, "null argument" );
	pt->testFreeBytes = bytes;
	return 0;
}
MVRT_EXPORT int mvrt_pt_set_profiling( mvrt_pt* pt, int enabled )
{
	REQUIRE( pt, "null argument" );
	pt->profiling = enabled != 0;
	return 0;
}
#ifdef MVRT_UTIL_STATS
// a diagnostic build's tallies behind the six of mvrt_pt_stats (tools/build_variant.sh util -DMVRT_UTIL_STATS), printed when MVRT_PRINT_UTIL is set
static int printUtilStats( const unsigned long long* stats, unsigned long long rays )
{
	// default stream, the three copies: mvrt_pt_get_stats, the only caller, has drained the slot streams and waited for its `stream`
	unsigned long long u[4];
	MVRT_HIP( hipMemcpy( u, stats + 8, sizeof( u ), hipMemcpyDeviceToHost ) );
	// u[0], u[1]: refill events and the lanes active right after them; u[2], u[3]: wave-iterations of the node-visit loop and
	// the lanes active in them
	fprintf( stderr, "[util] wave-iterations %llu, active-lane-iterations %llu (%.1f%% of lane slots); refill events %llu; rays %llu -> %.2f lane-iterations per ray\n", u[2], u[3],
			 100.0 * u[3] / ( 64.0 * ( u[2] ? u[2] : 1 ) ), u[0], rays, (double)u[3] / (double)( rays ? rays : 1 ) );
	unsigned long long c[2];
	MVRT_HIP( hipMemcpy( c, stats + 12, sizeof( c ), hipMemcpyDeviceToHost ) );
	fprintf( stderr, "[util] traversal waves: %.1f%% of their shader clocks in refill sections (result flush, ray loads, setup, hint replay)\n", 100.0 * (double)c[0] / (double)( c[1] ? c[1] : 1 ) );
	unsigned long long w[48];
	MVRT_HIP( hipMemcpy( w, stats + 16, sizeof( w ), hipMemcpyDeviceToHost ) );
	for( int k = 0; k <= MVRT_MAX_DEPTH; k++ )
		fprintf( stderr, "[util] stage %d: longest wave %llu iterations, waves %llu, longest ray %llu iterations\n", k, w[k], w[16 + k], w[32 + k] );
	return 0;
}
#endif
MVRT_EXPORT int mvrt_pt_reset_stats( mvrt_pt* pt )
{
	REQUIRE( pt, "null argument" );
	if( pt->drain() ) return 1;
	if( pt->statsBuf.p )
	{
		// default stream, behind the drain above; waited for, since the next step tallies on a non-blocking slot stream that does not wait for the default stream
		MVRT_HIP( hipMemset( pt->statsBuf.p, 0, 64 * 8 ) );
		MVRT_HIP( hipStreamSynchronize( nullptr ) );
	}
	pt->prof.collect();
	pt->prof.ms[0] = pt->prof.ms[1] = pt->prof.ms[2] = 0.0;
	pt->prof.traceLaunches = 0;
	return 0;
}
MVRT_EXPORT int mvrt_pt_get_stats( mvrt_pt* pt, void* stream, mvrt_pt_stats* out )
{
	REQUIRE( pt && out, "null argument" );
	memset( out, 0, sizeof( *out ) );
	if( pt->drain() ) return 1;
	MVRT_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
	if( pt->statsBuf.p )
	{
		unsigned long long s[6];
		MVRT_HIP( hipMemcpy( s, pt->statsBuf.p, sizeof( s ), hipMemcpyDeviceToHost ) ); // (default stream: behind the drain and the wait for `stream` above)
		out->rays = s[0];
		out->shadowRays = s[1];
		out->descents = s[2];
		out->shadowDescents = s[3];
		out->hits = s[4];
		out->samples = s[5];
#ifdef MVRT_UTIL_STATS
		if( getenv( "MVRT_PRINT_UTIL" ) && printUtilStats( pt->statsBuf.as<unsigned long long>(), s[0] ) ) return 1;
#endif
	}
	pt->prof.collect();
	out->traceLaunches = pt->prof.traceLaunches;
	out->traceKernelMs = pt->prof.ms[MVRT_K_TRACE];
	out->shadeKernelMs = pt->prof.ms[MVRT_K_SHADE];
	out->totalKernelMs = pt->prof.ms[0] + pt->prof.ms[1] + pt->prof.ms[2];
	return 0;
}
