// Stand-in for <optix_stubs.h>, used only by oracle/ref_build/ref_disney.cpp (test infrastructure).
// Intentionally empty: CUDABuffer.h (included by Probe.h) includes it, but ProbeData::BuildCDF calls
// no OptiX entry point, so no declaration is needed.
#pragma once
