// galois.hpp — internal interface between the host entry points of include/nttmul_galois.h
// (galois.cpp) and the launchers of galois.hip.  lib/libnttmul_galois.so only.
#pragma once
#include "galois_plan.hpp"
#include "rns.hpp"

namespace nttmul {

enum GaloisOp { kGaloisCoeff = 0, kGaloisNtt = 1, kGaloisNttMany = 2 };

constexpr uint32_t kGaloisMaxCount = 16;     // NTTMUL_GALOIS_MAX_COUNT
constexpr int kGaloisSlices = 4;             // slices of 256 words per workgroup (galois_dev.hpp)
constexpr uint32_t kGaloisStage = 1024;      // fewest words a k_galois_coeff workgroup stages
// the most a k_galois_coeff workgroup stages in LDS, of the 160 KiB of a compute unit.  Measured
// against 64 KiB (two workgroups per compute unit, twice the residue classes above it): level at
// n = 32768 on 32-bit words, 9 to 59 % faster at every other size that differs (DESIGN.md
// section 4).  Above 64 KiB the launcher raises the kernel's dynamic LDS limit.
constexpr size_t kGaloisLdsBytes = 128 << 10;

// the automorphisms of one k_galois_ntt_many launch, a kernel argument (by value)
struct GaloisKs {
  uint32_t k[kGaloisMaxCount];
};

// Per-device view of a Galois context: what a launch needs
struct GaloisTables {
  uint32_t logn = 0, limbs = 0;
  int word_bits = 0;
  const uint64_t *q = nullptr;  // device: the moduli, [limbs]
};

// One launch over a [batch][limbs][n] input on stream s (galois_dev.hpp), grid = (workgroups,
// limbs).  kv: the count automorphisms as the kernels take them: k^-1 mod 2n for kGaloisCoeff and
// kGaloisNttMany, k itself for kGaloisNtt (count 1 for the single calls).
hipError_t launch_galois(const GaloisTables &T, int op, void *out, const void *in,
                         const GaloisKs &kv, uint32_t count, size_t batch, hipStream_t s);
// The kernel launch_galois launches for (T, op): the dry run of the launching statement itself
hipError_t describe_galois(const GaloisTables &T, int op, std::string *out);

}  // namespace nttmul
