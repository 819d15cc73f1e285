// cone_probe.hip -- a user kernel on the cone-limited methods of include/mvrt/device.hpp (intersectCone / intersectConeEx, DeviceLod), loaded by
// tests/test_gpu_cone.py through ctypes.  Built by the test itself (hipcc --offload-arch=gfx950 -shared), with no contract flag.
#include <mvrt/device.hpp>

#define PROBE_BLOCK 64

// one ray per thread, SoA in / SoA out; stackMode 0: the thread's own stack, 1: the caller's stack in LDS.  hasLod: index and attrib through DeviceLod::lookup
// (index ~0 where the pyramid lacks the cell, 0 and zeros on a miss)
template <int STACK_MODE>
__global__ void __launch_bounds__( PROBE_BLOCK ) kProbeCone( mvrt_device_octree view, mvrt_device_lod lodView, int hasLod, uint64_t n, const float* rox, const float* roy,
															 const float* roz, const float* rdx, const float* rdy, const float* rdz, const float* coneA, const float* coneB, float* t,
															 int* nMajor, uint32_t* level, uint64_t* cellCode, uint32_t* descents, uint32_t* index, uint2* attrib )
{
	__shared__ mvrt::StackEntry lds[STACK_MODE == 1 ? PROBE_BLOCK * MVRT_DEVICE_MAX_LEVELS : 1];
	const mvrt::DeviceOctree oct( view );
	const uint64_t i = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if( i >= n ) return;
	const float3 ro = make_float3( rox[i], roy[i], roz[i] );
	const float3 rd = make_float3( rdx[i], rdy[i], rdz[i] );
	float tt, t2;
	int nm, nm2;
	uint32_t lv, lv2, de;
	uint64_t code, code2;
	if( STACK_MODE == 1 )
	{
		mvrt::StackEntry* stack = lds + threadIdx.x * view.levels;
		oct.intersectConeEx( stack, ro, rd, coneA[i], coneB[i], &tt, &nm, &lv, &code, &de );
		oct.intersectCone( stack, ro, rd, coneA[i], coneB[i], &t2, &nm2, &lv2, &code2 );
	}
	else
	{
		oct.intersectConeEx( ro, rd, coneA[i], coneB[i], &tt, &nm, &lv, &code, &de );
		oct.intersectCone( ro, rd, coneA[i], coneB[i], &t2, &nm2, &lv2, &code2 );
	}
	if( !( __float_as_uint( t2 ) == __float_as_uint( tt ) && nm2 == nm && lv2 == lv && code2 == code ) ) de = 0xFFFFFFFFu; // intersectCone must agree with intersectConeEx
	t[i] = tt;
	nMajor[i] = nm;
	level[i] = lv;
	cellCode[i] = code;
	descents[i] = de;
	if( hasLod )
	{
		const mvrt::DeviceLod lod( lodView );
		uint32_t idx = 0;
		uint2 a = make_uint2( 0u, 0u );
		if( lv != 0u )
		{
			if( lod.lookup( lv, code, &idx ) ) a = lod.attrib( lv, idx );
			else idx = 0xFFFFFFFFu;
		}
		index[i] = idx;
		attrib[i] = a;
	}
}

extern "C" int probe_cone( const mvrt_device_octree* view, const mvrt_device_lod* lod, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx,
						   const float* rdy, const float* rdz, const float* coneA, const float* coneB, float* t, int* nMajor, uint32_t* level, uint64_t* cellCode, uint32_t* descents,
						   uint32_t* index, uint32_t* attrib, int stackMode )
{
	if( view->structBytes != sizeof( mvrt_device_octree ) || view->levels > MVRT_DEVICE_MAX_LEVELS ) return -1;
	if( lod && ( lod->structBytes != sizeof( mvrt_device_lod ) || lod->levels != view->levels || !index || !attrib ) ) return -1;
	if( n == 0 ) return 0;
	mvrt_device_lod lv = {};
	if( lod ) lv = *lod;
	const dim3 grid( (unsigned)( ( n + PROBE_BLOCK - 1 ) / PROBE_BLOCK ) );
	if( stackMode == 1 )
		hipLaunchKernelGGL( kProbeCone<1>, grid, dim3( PROBE_BLOCK ), 0, 0, *view, lv, lod ? 1 : 0, n, rox, roy, roz, rdx, rdy, rdz, coneA, coneB, t, nMajor, level, cellCode, descents,
							index, (uint2*)attrib );
	else
		hipLaunchKernelGGL( kProbeCone<0>, grid, dim3( PROBE_BLOCK ), 0, 0, *view, lv, lod ? 1 : 0, n, rox, roy, roz, rdx, rdy, rdz, coneA, coneB, t, nMajor, level, cellCode, descents,
							index, (uint2*)attrib );
	if( hipGetLastError() != hipSuccess ) return -2;
	return hipDeviceSynchronize() == hipSuccess ? 0 : -3;
}
