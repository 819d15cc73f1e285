// stream_hold.hip -- what tests/streams.py loads: a non-blocking stream, and a kernel that keeps a stream busy for a given time, so that work queued behind it
// on that stream provably has not run yet while the host goes on (tests/test_gpu_stream_order.py).  The hold is bounded twice: by the wall clock and by a fixed
// number of iterations, so the kernel ends whatever the clock does.  One wave; plain C++ and compiler builtins; its only store is the elapsed tick count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SH_MAX_MS 250u
#define SH_MAX_ITERATIONS ( 1u << 18 ) // an iteration sleeps 127 * 64 clocks, a few microseconds: about a second at the most

__global__ void kHold( uint64_t ticks, uint32_t maxIterations, uint64_t* elapsedOut )
{
	const uint64_t t0 = wall_clock64();
	uint64_t t = t0;
	for( uint32_t i = 0; i < maxIterations && t - t0 < ticks; i++ )
	{
		__builtin_amdgcn_s_sleep( 127 );
		t = wall_clock64();
	}
	if( threadIdx.x == 0 ) elapsedOut[threadIdx.x] = t - t0;
}

static uint64_t* g_elapsed = nullptr; // one word, written by every hold (the value is not read back: the calibration times the hold from the host)

extern "C" int sh_stream_create_nonblocking( void** s )
{
	hipStream_t st = nullptr;
	const hipError_t e = hipStreamCreateWithFlags( &st, hipStreamNonBlocking );
	*s = (void*)st;
	return (int)e;
}

extern "C" int sh_stream_destroy( void* s ) { return (int)hipStreamDestroy( (hipStream_t)s ); }

extern "C" int sh_hold( void* stream, uint32_t ms )
{
	if( ms > SH_MAX_MS ) ms = SH_MAX_MS;
	if( !g_elapsed )
	{
		const hipError_t e = hipMalloc( (void**)&g_elapsed, sizeof( uint64_t ) );
		if( e != hipSuccess ) return (int)e;
	}
	int dev = 0, kHz = 0;
	if( hipGetDevice( &dev ) != hipSuccess || hipDeviceGetAttribute( &kHz, hipDeviceAttributeWallClockRate, dev ) != hipSuccess || kHz <= 0 ) kHz = 100000; // 100 MHz
	hipLaunchKernelGGL( kHold, dim3( 1 ), dim3( 64 ), 0, (hipStream_t)stream, (uint64_t)ms * (uint64_t)kHz, SH_MAX_ITERATIONS, g_elapsed );
	return (int)hipGetLastError();
}
