// Stand-in for <sutil/Exception.h>, used only by oracle/ref_build/ref_disney.cpp (test infrastructure).
// CUDABuffer.h (included by Probe.h) wraps its cudaMalloc/cudaMemcpy/cudaFree calls in these macros.
// They expand to nothing: ProbeData::BuildCDF never reaches a CUDABuffer member, and the built library
// imports no cuda* symbol (tests/test_oracle_reference_bsdf.py checks that).
// The real header also brings in <stdexcept>, which Probe.h relies on for std::runtime_error.
#pragma once
#include <stdexcept>
#define CUDA_CHECK(call)
#define CUDA_SYNC_CHECK()
#define OPTIX_CHECK(call)
