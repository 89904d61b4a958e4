/* kf_copy: the block copy of the keyframe store, the recovery switch and the ragged VO step (k_reloc.hip, k_vo.hip). */
#ifndef TB_KFCOPY_H
#define TB_KFCOPY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* Block copy of nbytes: 16-byte lanes where both sides are 16-byte aligned (every array of the store is, at a pitch that is a
 * multiple of 4), 4-byte lanes where both are 4-byte aligned, single bytes for the rest and for the tail. */
__device__ __forceinline__ void kf_copy(void* __restrict__ dst, const void* __restrict__ src, size_t nbytes, int tid) {
    const uintptr_t both = (uintptr_t)dst | (uintptr_t)src;
    size_t done = 0;
    if ((both & 15) == 0) {
        const size_t nv = nbytes >> 4;
        const uint4* S = reinterpret_cast<const uint4*>(src);
        uint4* D = reinterpret_cast<uint4*>(dst);
        for (size_t i = tid; i < nv; i += 256) D[i] = S[i];
        done = nv << 4;
    } else if ((both & 3) == 0) {
        const size_t nv = nbytes >> 2;
        const uint32_t* S = reinterpret_cast<const uint32_t*>(src);
        uint32_t* D = reinterpret_cast<uint32_t*>(dst);
        for (size_t i = tid; i < nv; i += 256) D[i] = S[i];
        done = nv << 2;
    }
    const uint8_t* S = reinterpret_cast<const uint8_t*>(src);
    uint8_t* D = reinterpret_cast<uint8_t*>(dst);
    for (size_t i = done + tid; i < nbytes; i += 256) D[i] = S[i];
}

#endif
