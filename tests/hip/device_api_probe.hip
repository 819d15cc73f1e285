// device_api_probe.hip -- a user kernel on include/mvrt/device.hpp, loaded by tests/test_gpu_device_api.py through ctypes.
// Built by the test itself (hipcc --offload-arch=gfx950 -shared), with no contract flag or with -ffp-contract=on.
#include <mvrt/device.hpp>

#define PROBE_BLOCK 64

// one ray per thread, SoA in / SoA out; stackMode 0: the thread's own stack, 1: the caller's stack in LDS
template <int STACK_MODE>
__global__ void __launch_bounds__( PROBE_BLOCK ) kProbeTrace( mvrt_device_octree view, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx,
															  const float* rdy, const float* rdz, const uint8_t* isShadow, float* t, int* nMajor, uint32_t* vIndex, uint32_t* descents )
{
	__shared__ mvrt::StackEntry lds[STACK_MODE == 1 ? PROBE_BLOCK * MVRT_DEVICE_MAX_LEVELS : 1];
	const mvrt::DeviceOctree oct( view );
	const uint64_t i = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if( i >= n ) return;
	const float3 ro = make_float3( rox[i], roy[i], roz[i] );
	const float3 rd = make_float3( rdx[i], rdy[i], rdz[i] );
	const bool sh = isShadow ? isShadow[i] != 0 : false;
	float tt;
	int nm;
	uint32_t vi, de;
	if( STACK_MODE == 1 )
		oct.intersectEx( lds + threadIdx.x * view.levels, ro, rd, &tt, &nm, &vi, sh, &de );
	else
		oct.intersectEx( ro, rd, &tt, &nm, &vi, sh, &de );
	t[i] = tt;
	nMajor[i] = nm;
	vIndex[i] = vi;
	descents[i] = de;
}

__global__ void kProbeAttrs( mvrt_device_octree view, uint32_t n, uchar4* color, float* emission, float* emissionRaw, uint32_t* hasEmission )
{
	const mvrt::DeviceOctree oct( view );
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if( i == 0 ) *hasEmission = oct.hasEmission() ? 1u : 0u;
	if( i >= n ) return;
	color[i] = oct.getVoxelColor( i );
	const float3 e = oct.getVoxelEmission( i, true ), r = oct.getVoxelEmission( i, false );
	emission[3 * i + 0] = e.x;
	emission[3 * i + 1] = e.y;
	emission[3 * i + 2] = e.z;
	emissionRaw[3 * i + 0] = r.x;
	emissionRaw[3 * i + 1] = r.y;
	emissionRaw[3 * i + 2] = r.z;
}

// mvrt::CameraPinhole on the device: px = n * 4 ints (x, y, W, H), fl = n * 4 floats (xo, yo, u0, u1); thinLens 0: shoot, else shootThinLens
__global__ void __launch_bounds__( PROBE_BLOCK ) kProbeCamera( mvrt::CameraPinhole cam, uint32_t n, const int* px, const float* fl, int thinLens, float* ro, float* rd )
{
	const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x;
	if( i >= n ) return;
	float3 o, d;
	if( thinLens )
		cam.shootThinLens( &o, &d, px[4 * i], px[4 * i + 1], fl[4 * i], fl[4 * i + 1], px[4 * i + 2], px[4 * i + 3], fl[4 * i + 2], fl[4 * i + 3] );
	else
		cam.shoot( &o, &d, px[4 * i], px[4 * i + 1], fl[4 * i], fl[4 * i + 1], px[4 * i + 2], px[4 * i + 3] );
	ro[3 * i + 0] = o.x;
	ro[3 * i + 1] = o.y;
	ro[3 * i + 2] = o.z;
	rd[3 * i + 0] = d.x;
	rd[3 * i + 1] = d.y;
	rd[3 * i + 2] = d.z;
}

extern "C" int probe_trace( const mvrt_device_octree* view, uint64_t n, const float* rox, const float* roy, const float* roz, const float* rdx, const float* rdy, const float* rdz,
							const uint8_t* isShadow, float* t, int* nMajor, uint32_t* vIndex, uint32_t* descents, int stackMode )
{
	if( view->structBytes != sizeof( mvrt_device_octree ) || view->levels > MVRT_DEVICE_MAX_LEVELS ) return -1;
	if( n == 0 ) return 0;
	const dim3 grid( (unsigned)( ( n + PROBE_BLOCK - 1 ) / PROBE_BLOCK ) );
	if( stackMode == 1 )
		hipLaunchKernelGGL( kProbeTrace<1>, grid, dim3( PROBE_BLOCK ), 0, 0, *view, n, rox, roy, roz, rdx, rdy, rdz, isShadow, t, nMajor, vIndex, descents );
	else
		hipLaunchKernelGGL( kProbeTrace<0>, grid, dim3( PROBE_BLOCK ), 0, 0, *view, n, rox, roy, roz, rdx, rdy, rdz, isShadow, t, nMajor, vIndex, descents );
	if( hipGetLastError() != hipSuccess ) return -2;
	return hipDeviceSynchronize() == hipSuccess ? 0 : -3;
}

extern "C" int probe_attrs( const mvrt_device_octree* view, uint32_t n, uchar4* color, float* emission, float* emissionRaw, uint32_t* hasEmission )
{
	if( view->structBytes != sizeof( mvrt_device_octree ) ) return -1;
	hipLaunchKernelGGL( kProbeAttrs, dim3( ( n + 255 ) / 256 + 1 ), dim3( 256 ), 0, 0, *view, n, color, emission, emissionRaw, hasEmission );
	if( hipGetLastError() != hipSuccess ) return -2;
	return hipDeviceSynchronize() == hipSuccess ? 0 : -3;
}

// cam15 on the host, everything else in device memory
extern "C" int probe_camera( const float* cam15, uint32_t n, const int* px, const float* fl, int thinLens, float* ro, float* rd )
{
	if( n == 0 ) return 0;
	hipLaunchKernelGGL( kProbeCamera, dim3( ( n + PROBE_BLOCK - 1 ) / PROBE_BLOCK ), dim3( PROBE_BLOCK ), 0, 0, mvrt::CameraPinhole( cam15 ), n, px, fl, thinLens, ro, rd );
	if( hipGetLastError() != hipSuccess ) return -2;
	return hipDeviceSynchronize() == hipSuccess ? 0 : -3;
}

// the same members on the host (they are __host__ __device__): all pointers in host memory, no HIP call
extern "C" void probe_camera_host( const float* cam15, uint32_t n, const int* px, const float* fl, int thinLens, float* ro, float* rd )
{
	const mvrt::CameraPinhole cam( cam15 );
	for( uint32_t i = 0; i < n; i++ )
	{
		float3 o, d;
		if( thinLens )
			cam.shootThinLens( &o, &d, px[4 * i], px[4 * i + 1], fl[4 * i], fl[4 * i + 1], px[4 * i + 2], px[4 * i + 3], fl[4 * i + 2], fl[4 * i + 3] );
		else
			cam.shoot( &o, &d, px[4 * i], px[4 * i + 1], fl[4 * i], fl[4 * i + 1], px[4 * i + 2], px[4 * i + 3] );
		ro[3 * i + 0] = o.x;
		ro[3 * i + 1] = o.y;
		ro[3 * i + 2] = o.z;
		rd[3 * i + 0] = d.x;
		rd[3 * i + 1] = d.y;
		rd[3 * i + 2] = d.z;
	}
}
