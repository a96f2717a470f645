// vmp_dev.h — address-space macros, streaming stores and the wave-level
// helpers (ballot, readlane, wave barrier) every env kernel is written with.
// Restates nothing of the reference. Included by the other kernel headers of
// vmp_kernels.hip.
#ifndef VMP_DEV_H
#define VMP_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// Pointers into LDS carry address space 3 explicitly: 32-bit addresses (half
// the SGPRs of generic pointers) and ds_* instructions without relying on
// address-space inference through the helpers.
#define LDSP __attribute__((address_space(3)))

// Minimum waves per SIMD the env kernel is register-allocated for
// (__launch_bounds__ 2nd argument); measured choice, see DESIGN.md.
#ifndef VMP_WAVES_PER_EU
#define VMP_WAVES_PER_EU 2
#endif
#ifndef VMP_WAVES_PER_EU_ONE  // the per-step (k_steps == 1) instantiation
#define VMP_WAVES_PER_EU_ONE 3
#endif

namespace vmp {

// Global (address space 1) views of HBM pointers. Pointers read out of the
// EnvParams / StepOut structs are generic, and generic accesses compile to
// FLAT instructions, which count in lgkmcnt as well as vmcnt: every later
// s_waitcnt lgkmcnt for an LDS access then also waits for them to complete
// (in k_env_big the mid-step state stores stalled every following LDS wait).
#define GLBP __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ T GLBP *gptr(T *p) {
  return (T GLBP *)p;
}

#ifdef VMP_CHECK_QUIET
// quiet-bit check build: quiet steps in which some pending VM fit a PM
// (read and reset by quiet_violations_take in vmp_kernels.hip: a __device__
// global is per code object, so it and its users stay in that one unit)
__device__ unsigned long long g_quiet_violations;
#endif

// Register row s of lane ln (slot v = 64 s + ln) in the blocked VM words of
// a wave kernel: the slot word's index (= vm_slot_idx(v)), + 64 for the time
// word. vm_pitch pads the env's blocks to the kernel's rows, so a padded slot
// (v >= V) reads padding inside the env's pitch, never used.
__device__ __forceinline__ int vw_row(int s, int ln) { return (s << 7) + ln; }

// Streaming stores (obs / state written once per launch, not re-read by it).
#define ST_NT(ptr, val) __builtin_nontemporal_store((val), gptr(ptr))

// ------------------------------------------------------------ wave utils --
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// An LDS base the compiler cannot tie to earlier address arithmetic: the
// pointers make_lds derives from it at a late use are recomputed there instead
// of being kept live (and spilled) from the prologue.
__device__ __forceinline__ char LDSP *opaque_base(char LDSP *b) {
  uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)b);  // 32-bit
  asm volatile("" : "+s"(x));
  return (char LDSP *)(uintptr_t)x;
}
// The lane id recomputed where the compiler cannot tie it to lane_id(): slot
// indices s*64 + lane built from it in a late phase (the obs / state stores)
// are not the prologue's, which the register allocator otherwise keeps live
// (spilled to scratch) from the loads at entry to the stores at exit.
__device__ __forceinline__ int fresh_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int below(uint64_t m, int lane) {
  return __popcll(m & ((1ull << lane) - 1ull));
}
// LDS hand-off between lanes of ONE wave: order the accesses, no s_barrier.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t rdlane(uint32_t x, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)x, l);
}

}  // namespace vmp

#endif  // VMP_DEV_H
