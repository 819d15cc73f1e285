// devbuf.h -- DevBuf, the one owner of the device memory this library allocates for itself (role of hipUtil.hpp:48-74 Buffer).
// Host code only.  Every allocation of the library goes through DevBuf::alloc, so the tallies and the failure hook below see all of them
// (mvrt_test_allocation_state / mvrt_test_fail_allocation, mvrt.h); mvrt_malloc / mvrt_free are the caller's memory and pass by.
#pragma once
#include <atomic>

#include "mvrt_common.h"

struct DevBufState // process-wide
{
	std::atomic<uint64_t> liveBuffers{ 0 }, liveBytes{ 0 }, totalAllocs{ 0 };
	std::atomic<uint64_t> peakBytes{ 0 }; // the largest liveBytes since mvrt_test_peak_bytes last reset it
};
inline DevBufState g_devBufState;
inline thread_local int64_t g_devBufFailIn = 0; // n > 0: the n-th alloc from now on this thread fails, then the hook is off again

struct DevBuf // move-only
{
	void* p = nullptr;
	uint64_t bytes = 0;
	int alloc( uint64_t b ) // releases what it holds first; on failure it holds nothing
	{
		release();
		g_devBufState.totalAllocs++;
		if( g_devBufFailIn > 0 && --g_devBufFailIn == 0 )
		{
			mvrtSetError( "allocation of %llu bytes refused by mvrt_test_fail_allocation", (unsigned long long)b );
			return 1;
		}
		MVRT_HIP( hipMalloc( &p, b ? b : 1 ) );
		bytes = b;
		g_devBufState.liveBuffers++;
		const uint64_t live = ( g_devBufState.liveBytes += b );
		for( uint64_t peak = g_devBufState.peakBytes; live > peak && !g_devBufState.peakBytes.compare_exchange_weak( peak, live ); ) {}
		return 0;
	}
	void release()
	{
		if( p )
		{
			(void)hipFree( p );
			g_devBufState.liveBuffers--;
			g_devBufState.liveBytes -= bytes;
		}
		p = nullptr;
		bytes = 0;
	}
	~DevBuf() { release(); }
	DevBuf() {}
	DevBuf( DevBuf&& o ) noexcept : p( o.p ), bytes( o.bytes )
	{
		o.p = nullptr;
		o.bytes = 0;
	}
	DevBuf& operator=( DevBuf&& o ) noexcept
	{
		if( this != &o )
		{
			release();
			p = o.p;
			bytes = o.bytes;
			o.p = nullptr;
			o.bytes = 0;
		}
		return *this;
	}
	DevBuf( const DevBuf& ) = delete;
	DevBuf& operator=( const DevBuf& ) = delete;
	template <class T> T* as() const { return (T*)p; }
};

// hipcub's two calls: ask for the size of the temporary storage, allocate it, run.  Waits for the stream, since the storage is released on return
template <class Call> int withCubTemp( hipStream_t st, Call call )
{
	size_t tmpBytes = 0;
	MVRT_HIP( call( nullptr, tmpBytes ) );
	DevBuf tmp;
	if( tmp.alloc( tmpBytes ) ) return 1;
	MVRT_HIP( call( tmp.p, tmpBytes ) );
	MVRT_HIP( hipStreamSynchronize( st ) );
	return 0;
}
