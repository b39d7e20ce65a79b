// vq_bf16.h — the one fp32 -> bf16 rounding of the bf16-operand modes (DESIGN.md §14 Vec3 inference, §23 scalar decode).
#pragma once

#include <cstdint>

namespace v3b {

// fp32 -> bf16 bits, round to nearest even (NaN stays a quiet NaN); what torch's .to(torch.bfloat16) does
__host__ __device__ inline uint32_t bf16_bits(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

}  // namespace v3b
