// surface_weld.h -- what kernels_surface.hip shares with kernels_smooth.hip: the corner tables of a voxel face, and the host steps from a handle's masks to the
// welded mesh (the masks and their count, the face offsets, the emit launch, the SurfaceWeld record).  The functions are defined in kernels_surface.hip; the rules they
// follow are those of mvrt_svo_surface_mesh (mvrt.h).
#pragma once
#include "launch.h"
#include "voxel_passes.h"

// corner number -> offset (the reference's numbering): 0 (0,0,0) 1 (1,0,0) 2 (1,0,1) 3 (0,0,1) 4 (0,1,0) 5 (1,1,0) 6 (1,1,1) 7 (0,1,1)
MVRT_HDI uint32_t cornerX( uint32_t c ) { return ( 0x66u >> c ) & 1u; }
MVRT_HDI uint32_t cornerY( uint32_t c ) { return ( 0xF0u >> c ) & 1u; }
MVRT_HDI uint32_t cornerZ( uint32_t c ) { return ( 0xCCu >> c ) & 1u; }
// face d, corner k -> corner number: -Y 3,2,1,0  +Y 4,5,6,7  -Z 0,1,5,4  +X 1,2,6,5  +Z 2,3,7,6  -X 3,0,4,7 (three bits each, corner 0 lowest)
MVRT_HDI uint32_t faceCorner( uint32_t d, uint32_t k )
{
	const uint64_t lo = 03u | 02u << 3 | 01u << 6 | 00u << 9 | ( 04ull | 05u << 3 | 06u << 6 | 07u << 9 ) << 12 | ( 00ull | 01u << 3 | 05u << 6 | 04u << 9 ) << 24;
	const uint64_t hi = 01u | 02u << 3 | 06u << 6 | 05u << 9 | ( 02ull | 03u << 3 | 07u << 6 | 06u << 9 ) << 12 | ( 03ull | 00u << 3 | 04u << 6 | 07u << 9 ) << 24;
	return (uint32_t)( ( d < 3u ? lo >> ( 12u * d ) : hi >> ( 12u * ( d - 3u ) ) ) >> ( 3u * k ) ) & 7u;
}

// the kernel kSurfaceEmit over the voxels of s: offs = the n + 1 exclusive face offsets of `masks`; any output may be null.  Not synchronised.
int surfaceLaunchEmit( const SurfaceSource& s, const uint8_t* masks, const uint64_t* offs, uint32_t* faceVoxel, uint8_t* faceDir, float* positions, uint64_t* keys, uint32_t* vals,
				hipStream_t st );
// the exposure masks, or a caller's `given` masks without bits 6-7, into scratch of n + 1 bytes (the last one 0, so that the scan below yields offs[n]) and the
// sum of the popcounts, on the host when this returns
int surfaceScratchMasks( const SurfaceSource& s, const uint8_t* given, DevBuf& masks, uint64_t* nFaces, hipStream_t st );
int surfaceScanOffsets( const SurfaceSource& s, const DevBuf& masks, DevBuf& offs, hipStream_t st );

// The weld of a list of quads (unit faces or merged rectangles): the corners sorted by key with their numbers (quad * 4 + k), rank + 1 of every sorted corner among
// the distinct keys, and the two counts.  Left empty where there is no corner.
struct SurfaceWeld
{
	DevBuf keys, vals, rank1;
	uint32_t nCorners = 0, nVertices = 0;
};
// from the keys and numbers of nCorners >= 1 corners (keysA / valsA are released): radix sort, head flags, inclusive scan.  The counts are on the host when this returns
int surfaceBuildWeld( const SurfaceSource& s, DevBuf& keysA, DevBuf& valsA, uint32_t nCorners, SurfaceWeld* w, hipStream_t st );
// indices[quad * 4 + k] and the vertices of a weld with corners; either may be null.  Not synchronised.
int surfaceWriteWeld( const SurfaceSource& s, const SurfaceWeld& w, uint32_t* indicesDev, float* verticesDev, hipStream_t st );
