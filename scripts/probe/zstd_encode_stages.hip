// zstd_encode_stages.hip — k_zstd_encode_blocks (aggfly_amd/csrc/afhip_zstd_encode_kernels.h) compiled to stop after its first stage
// (-DAFZE_STOP_AFTER=1: matches), after its second (=2: matches and sequences) or not at all, each as a small library of its own with
// one entry, so that scripts/probe/zstd_encode_stages.py can time the three on the buffers of the production route: the differences
// are the stages' shares of the kernel.  The production library is not built with the switch.
//   hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -I aggfly_amd/csrc [-DAFZE_STOP_AFTER=k] scripts/probe/zstd_encode_stages.hip -o ...
#include "afhip_zstd_encode_kernels.h"

extern "C" int probe_zstd_encode_blocks(const void* in_dev, const void* blocks_dev, long long n_blocks, void* scratch_dev, void* slots_dev,
                                        int* csize_dev, void* stream) {
    using namespace afhip;
    hipLaunchKernelGGL(k_zstd_encode_tables, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint8_t*)scratch_dev);
    const dim3 grid((unsigned)(n_blocks < 65535 ? n_blocks : 65535), (unsigned)((n_blocks + 65534) / 65535));
    hipLaunchKernelGGL(k_zstd_encode_blocks, grid, dim3(64), 0, (hipStream_t)stream, (const uint8_t*)in_dev, (const ZstdEncodeBlock*)blocks_dev,
                       (int64_t)n_blocks, (uint8_t*)scratch_dev, (uint8_t*)slots_dev, csize_dev);
    return (int)hipGetLastError();
}
