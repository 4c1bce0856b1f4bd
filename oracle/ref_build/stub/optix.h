// Stand-in for <optix.h>, used only by oracle/ref_build/ref_disney.cpp and ref_device.cpp (test infrastructure).
// Declares the CUDA driver types and OptixTraversableHandle, the one OptiX type the pinned headers
// name: LaunchParams.h (included by Disney.cuh) has a field of that type.  No function pinned from
// Disney.cuh or Probe.h reads the field or calls into OptiX, so nothing here defines OptiX behaviour;
// ref_device.cpp keeps its scene record in the field and gets it back in optixTrace (stub/optix_device.h).
#pragma once
#include <cuda.h>
typedef unsigned long long OptixTraversableHandle;
