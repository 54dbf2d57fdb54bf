// Counter-based random numbers: the splitmix64 construction of diffudf_amd/synth.py.  ONE copy, so that the sampler (dudf_sample.hip)
// and the point-cloud proposals (dudf_pointcloud.hip) cannot drift from each other or from the numpy oracles.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ __forceinline__ uint64_t dudf_splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform in [0, 1): a pure function of (stream key, counter)
__device__ __forceinline__ double dudf_uniform01(uint64_t key, uint64_t idx) {
    uint64_t b = dudf_splitmix64(idx ^ key);
    b = dudf_splitmix64(b + key);
    return (double)(b >> 11) * (1.0 / 9007199254740992.0);
}
