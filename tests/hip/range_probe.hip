// range_probe.hip -- a user kernel on the distance-limited methods of include/mvrt/device.hpp, loaded by tests/test_gpu_range.py through ctypes.
// Built by the test itself (hipcc --offload-arch=gfx950 -shared), with no contract flag or with -ffp-contract=on.
#include <mvrt/device.hpp>

#define PROBE_BLOCK 64

// one ray per thread, SoA in / SoA out; stackMode 0: the thread's own stack, 1: the caller's stack in LDS.  occluded[i] = occluded( ro, rd, tMax ) of the same ray
template <int STACK_MODE>
__global__ void __launch_bounds__( PROBE_BLOCK ) kProbeRange( mvrt_device_octree view, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx,
															  const float* rdy, const float* rdz, const uint8_t* isShadow, const float* tMax, float* t, int* nMajor, uint32_t* vIndex,
															  uint32_t* descents, uint8_t* occluded )
{
	__shared__ mvrt::StackEntry lds[STACK_MODE == 1 ? PROBE_BLOCK * MVRT_DEVICE_MAX_LEVELS : 1];
	const mvrt::DeviceOctree oct( view );
	const uint64_t i = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if( i >= n ) return;
	const float3 ro = make_float3( rox[i], roy[i], roz[i] );
	const float3 rd = make_float3( rdx[i], rdy[i], rdz[i] );
	const bool sh = isShadow ? isShadow[i] != 0 : false;
	float tt, t2;
	int nm, nm2;
	uint32_t vi, vi2, de;
	bool occ;
	if( STACK_MODE == 1 )
	{
		mvrt::StackEntry* stack = lds + threadIdx.x * view.levels;
		oct.intersectRangeEx( stack, ro, rd, tMax[i], &tt, &nm, &vi, sh, &de );
		oct.intersectRange( stack, ro, rd, tMax[i], &t2, &nm2, &vi2, sh );
		occ = oct.occluded( stack, ro, rd, tMax[i] );
	}
	else
	{
		oct.intersectRangeEx( ro, rd, tMax[i], &tt, &nm, &vi, sh, &de );
		oct.intersectRange( ro, rd, tMax[i], &t2, &nm2, &vi2, sh );
		occ = oct.occluded( ro, rd, tMax[i] );
	}
	if( !( __float_as_uint( t2 ) == __float_as_uint( tt ) && nm2 == nm && vi2 == vi ) ) de = 0xFFFFFFFFu; // intersectRange must agree with intersectRangeEx
	t[i] = tt;
	nMajor[i] = nm;
	vIndex[i] = vi;
	descents[i] = de;
	occluded[i] = occ ? 1 : 0;
}

extern "C" int probe_range( const mvrt_device_octree* view, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz,
							const uint8_t* isShadow, const float* tMax, float* t, int* nMajor, uint32_t* vIndex, uint32_t* descents, uint8_t* occluded, int stackMode )
{
	if( view->structBytes != sizeof( mvrt_device_octree ) || view->levels > MVRT_DEVICE_MAX_LEVELS ) return -1;
	if( n == 0 ) return 0;
	const dim3 grid( (unsigned)( ( n + PROBE_BLOCK - 1 ) / PROBE_BLOCK ) );
	if( stackMode == 1 )
		hipLaunchKernelGGL( kProbeRange<1>, grid, dim3( PROBE_BLOCK ), 0, 0, *view, n, rox, roy, roz, rdx, rdy, rdz, isShadow, tMax, t, nMajor, vIndex, descents, occluded );
	else
		hipLaunchKernelGGL( kProbeRange<0>, grid, dim3( PROBE_BLOCK ), 0, 0, *view, n, rox, roy, roz, rdx, rdy, rdz, isShadow, tMax, t, nMajor, vIndex, descents, occluded );
	if( hipGetLastError() != hipSuccess ) return -2;
	return hipDeviceSynchronize() == hipSuccess ? 0 : -3;
}
