/*
 * Stand-in for "Orochi/Orochi.h", on the include path of the `ref` build only (oracle/Makefile).  The reference's hipUtil.hpp (Buffer, Shader) and
 * the host halves of renderCommon.hpp (HDRI::load / loadPrimary / cleanUp) and pmjSampler.hpp (PMJSampler::setup( true, ... ) / cleanUp) name the
 * Orochi driver API.  This file supplies the types and no-op definitions that make those members parse; oracle/ref_shim_render.cpp calls none of
 * them -- it never constructs a Buffer or a Shader, never calls HDRI::load, and calls PMJSampler::setup with isGPU == false only -- so nothing a
 * test compares depends on what stands here (the stand-in rule).  Our own text.
 *
 * It also includes the C and C++ headers that hipUtil.hpp uses without including them (FILE, printf, memcpy, malloc, std::map, std::max), and adds
 * the one overload that hipUtil.hpp:55 needs where int64_t is long (LP64): std::max( int64_t, 1LL ) has no common type there.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>

namespace std
{
inline long long max( long a, long long b ) { return a < b ? b : (long long)a; }
} // namespace std

typedef void* oroDeviceptr;
typedef struct standin_oroStream* oroStream;
typedef struct standin_oroModule* oroModule;
typedef struct standin_oroFunction* oroFunction;
typedef struct standin_orortcProgram* orortcProgram;
enum oroError
{
	oroSuccess = 0,
	oroErrorUnknown = 999
};
enum orortcResult
{
	ORORTC_SUCCESS = 0,
	ORORTC_ERROR_INTERNAL_ERROR = 11
};

// every call fails or does nothing: there is no device behind this header
inline oroError oroMalloc( oroDeviceptr* p, size_t ) { *p = 0; return oroErrorUnknown; }
inline oroError oroFree( oroDeviceptr ) { return oroErrorUnknown; }
inline oroError oroMemcpyHtoDAsync( oroDeviceptr, const void*, size_t, oroStream ) { return oroErrorUnknown; }
inline oroError oroStreamSynchronize( oroStream ) { return oroErrorUnknown; }
inline oroError oroModuleLoadData( oroModule* m, const void* ) { *m = 0; return oroErrorUnknown; }
inline oroError oroModuleUnload( oroModule ) { return oroErrorUnknown; }
inline oroError oroModuleGetFunction( oroFunction* f, oroModule, const char* ) { *f = 0; return oroErrorUnknown; }
inline oroError oroModuleLaunchKernel( oroFunction, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, oroStream, void**, void** )
{
	return oroErrorUnknown;
}
inline orortcResult orortcCreateProgram( orortcProgram* p, const char*, const char*, int, const char**, const char** ) { *p = 0; return ORORTC_ERROR_INTERNAL_ERROR; }
inline orortcResult orortcCompileProgram( orortcProgram, int, const char** ) { return ORORTC_ERROR_INTERNAL_ERROR; }
inline orortcResult orortcGetProgramLogSize( orortcProgram, size_t* n ) { *n = 0; return ORORTC_ERROR_INTERNAL_ERROR; }
inline orortcResult orortcGetProgramLog( orortcProgram, char* ) { return ORORTC_ERROR_INTERNAL_ERROR; }
inline orortcResult orortcGetCodeSize( orortcProgram, size_t* n ) { *n = 0; return ORORTC_ERROR_INTERNAL_ERROR; }
inline orortcResult orortcGetCode( orortcProgram, char* ) { return ORORTC_ERROR_INTERNAL_ERROR; }
inline orortcResult orortcDestroyProgram( orortcProgram* ) { return ORORTC_ERROR_INTERNAL_ERROR; }
