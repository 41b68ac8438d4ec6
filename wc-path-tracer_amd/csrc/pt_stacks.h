/* pt_stacks.h -- the traversal stacks: PrivateStack (scratch) and LdsStack (LDS with a scratch spill).
 * Part of pt_device.h. */
#ifndef WCPT_PT_STACKS_H
#define WCPT_PT_STACKS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wcpt::dev {

/* Traversal stacks; entries = (node index, box entry distance t0) of deferred far children.
 *
 * PrivateStack keeps the entries in private (scratch) memory: simple, but every push/pop is a VMEM store/load
 * that the per-XCD L2 cannot hold at full occupancy (measured: ~6 GB of writes per 1080p atrium frame).
 * LdsStack keeps the first N entries in LDS, lane-interleaved ([entry][64 lanes] of 8-byte words: one
 * conflict-free ds_write_b64 / ds_read_b64 per wave), and only entries N..N+SPILL-1 in scratch. */
/* The entry storage is a separate private array owned by the caller (`mem` / `spill` point at it) so that the
 * stack pointer itself stays in a register: with the arrays inside the struct, the dynamic array indexing kept
 * the whole struct -- sp included -- in scratch, and every push/pop paid a scratch round trip for sp. */
typedef __attribute__((address_space(5))) uint64_t* priv_u64_ptr;
typedef __attribute__((address_space(3))) uint64_t* lds_u64_ptr;

template <int N>
struct PrivateStack {
    priv_u64_ptr mem; /* caller's private uint64_t[N], entries (node index | t0 bits << 32) */
    int sp;
    __device__ __forceinline__ void reset() { sp = 0; }
    __device__ __forceinline__ bool empty() const { return sp == 0; }
    __device__ __forceinline__ bool push(uint32_t i, float t)
    {
        if (sp >= N) return false;
        mem[sp] = (uint64_t)i | ((uint64_t)__float_as_uint(t) << 32);
        sp++;
        return true;
    }
    __device__ __forceinline__ void pop(uint32_t& i, float& t)
    {
        sp--;
        const uint64_t e = mem[sp];
        i = (uint32_t)e;
        t = __uint_as_float((uint32_t)(e >> 32));
    }
};

/* Entries are packed (node index | t0 bits << 32). The two storage classes are typed by address space so that
 * the compiler emits ds_read/ds_write for the LDS part and scratch_* for the spill instead of merging the two
 * into one flat access. */
template <int N, int SPILL>
struct LdsStack {
    lds_u64_ptr base;   /* &lds[0][lane] */
    priv_u64_ptr spill; /* caller's private uint64_t[SPILL] */
    int sp;
    __device__ __forceinline__ void reset() { sp = 0; }
    __device__ __forceinline__ bool empty() const { return sp == 0; }
    __device__ __forceinline__ bool push(uint32_t i, float t)
    {
        const uint64_t e = (uint64_t)i | ((uint64_t)__float_as_uint(t) << 32);
        if (sp < N) {
            base[sp * 64] = e;
        } else if (sp < N + SPILL) {
            spill[sp - N] = e;
        } else {
            return false;
        }
        sp++;
        return true;
    }
    __device__ __forceinline__ void pop(uint32_t& i, float& t)
    {
        sp--;
        uint64_t e;
        if (sp < N) {
            e = base[sp * 64];
        } else {
            e = spill[sp - N];
#if defined(__gfx9__)
            /* wait for the spill load inside its (rare) branch: otherwise the LDS read of the other lanes, which
             * writes the same registers, waits for vmcnt(0) on every pop -- and so for every store still in flight.
             * The immediate is the gfx9 s_waitcnt encoding (gfx950 is gfx9); other generations lay the counters out
             * differently and get no explicit wait. Measured c4 -1.2 % alone, c3 -1.4 % alone, and with the deferred
             * hit stores (pt_wavefront.hip, kModeIdlePend) c3 -2.9 % / c4 -2.8 % (profiles/r05_store_wait_ab.log). */
            __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0), expcnt/lgkmcnt untouched (gfx9 encoding) */
#endif
        }
        i = (uint32_t)e;
        t = __uint_as_float((uint32_t)(e >> 32));
    }
};

} // namespace wcpt::dev

#endif /* WCPT_PT_STACKS_H */
