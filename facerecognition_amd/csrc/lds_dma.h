// Device primitives of the LDS-DMA kernels, each written once: buffer resources, the 16-byte LDS-DMA in its two
// flavours, counted waits, the LDS-only barrier, the 16-bit pack and the recomputed lane / thread ids.  Included by
// kernel files only (inline asm: not for the host-only units that see common.h).
#pragma once
#include "common.h"

namespace fr {

typedef int v4i32 __attribute__((ext_vector_type(4)));             // a buffer resource as an "s" asm operand
typedef __attribute__((address_space(3))) void lds_void;           // the LDS pointer type of the DMA builtin
constexpr uint32_t OOB = 0x80000000u;  // a buffer offset past num_records: the load (or DMA) returns zeros -- no
                                       // select, no zero page for padding taps, halo columns and rows past the end
constexpr int RSRC_WORD3 = 0x00020000;  // resource word 3 of a raw buffer (stride 0, offsets in bytes): 32-bit data
                                        // format, no swizzle; the range check is offset < num_records

// num_records is a 32-bit byte count: a size computed in size_t that may pass 2 GiB is clamped before the narrowing
// (offsets stay below 2^31 in any case: OOB is the first value out of every range)
__device__ __forceinline__ uint32_t clamp31(size_t bytes) { return (uint32_t)min((size_t)0x7fffffff, bytes); }

// `bytes` of memory at p, for the builtin buffer loads, stores and dma16 / dma16s ...
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, RSRC_WORD3);
}
// ... and the same four words built by hand, for the asm DMAs
__device__ __forceinline__ v4i32 buffer_rsrc_words(const void* p, uint32_t bytes) {
    const uint64_t a = (uint64_t)p;
    return (v4i32){(int)(uint32_t)a, (int)((a >> 32) & 0xffff), (int)bytes, RSRC_WORD3};
}

// ---- 16-byte LDS-DMA (buffer_load_dwordx4 ... lds): lane l's 16 bytes at buffer offset voff land at lds + 16 l, so
// a wave instruction fills 1 KiB of LDS linearly and any layout is a permutation of the per-lane SOURCE offsets.
//
// Compiler-visible flavour: the builtin.  The compiler knows about the LDS write: its waitcnt pass puts a vmcnt in
// front of this wave's later LDS accesses, and __syncthreads() drains the DMA for the other waves.  A kernel counts
// vmcnt itself (wait_vm<N>() and a raw barrier) only to wait for less than everything in flight.
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, const char* lds, uint32_t voff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds, 16, voff, 0, 0, 0);
}
// ... with a wave-uniform byte offset in soffset: it shifts the memory address only (the instruction's immediate
// offset would also shift the LDS destination)
__device__ __forceinline__ void dma16s(__amdgpu_buffer_rsrc_t rsrc, const char* lds, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)lds, 16, voff, soff, 0, 0);
}

// Compiler-invisible flavour: the same instruction from inline asm.  The compiler does not see the LDS write, so its
// waitcnt pass puts no vmcnt(0) -- the whole DMA, and every output store with it -- in front of later LDS accesses
// that do not touch the slots in flight.  The caller owes every wait: a counted wait_vm<N>() (N = the VMEM operations
// it issued after the DMA it waits for) and a barrier before the data is read, and a wait_vm<0>() before the block
// ends or reuses the LDS.  Between those, the counts must see only what the kernel itself issued: registers loaded
// from global memory earlier are consumed (asm volatile("" : "+v"(x))) before the first DMA.  m0 is reserved to the
// compiler, hence the pragma; a kernel that uses this DMA uses m0 for nothing else.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma16_asm(const v4i32& rsrc, uint32_t lds_addr, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
                 :
                 : "v"(voff), "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane(lds_addr))
                 : "memory", "m0");
}
// ... with the wave-uniform soffset (memory address only, as dma16s)
__device__ __forceinline__ void dma16_asm(const v4i32& rsrc, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :
                 : "v"(voff), "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane(lds_addr)), "s"(soff)
                 : "memory", "m0");
}
#pragma clang diagnostic pop

// At most N VMEM operations of this wave still in flight (N <= 63, the vmcnt field)
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// A barrier that waits for this wave's LDS operations only: __syncthreads() also drains vmcnt, i.e. every DMA and
// store in flight
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Four floats -> four bf16 / f16 (common.h's pack2: RNE, f16 saturating)
template <bool F16>
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
    if (F16) return make_uint2(pack2_f16(a, b), pack2_f16(c, d));
    return make_uint2(pack2_bf16(a, b), pack2_bf16(c, d));
}

// 16-B chunk of a 128-B LDS row after the XOR swizzle with (row >> 1) & 7: the MFMA-fragment ds_read_b128 of 16
// consecutive rows is bank-conflict free.  Applied to the per-lane DMA source chunk and to the fragment reads.
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// The lane id recomputed where it is used (v_mbcnt in volatile asm: never hoisted, CSE'd or kept live across a
// loop).  A long-lived copy of threadIdx.x, and the loop-invariant per-lane addresses derived from it, stay live for
// the whole kernel and get spilled; each scratch reload then waits for every outstanding VMEM load (vmcnt(0)), i.e.
// drains the weight prefetch ring.
__device__ __forceinline__ int fresh_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// ... and the thread id of a 1-D block built on it: the wave's base from a scalar read
__device__ __forceinline__ int fresh_tid() {
    return (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63) + fresh_lane();
}
// threadIdx.x through an empty asm: the cheaper form, enough where only the addresses computed from the id must be
// recomputed at their use instead of being hoisted to the kernel's start and spilled across the K loops
__device__ __forceinline__ int opaque_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

}  // namespace fr
