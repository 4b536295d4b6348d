// mac.hpp — internal interface between the host entry points of include/nttmul_mac.h
// (nttmul.cpp, NTTMUL_MAC blocks) and the launchers of mac.hip.  lib/libnttmul_mac.so only.
#pragma once
#include "launch.hpp"

namespace nttmul {

// c[p] = INTT(sum_t NTT(a[p][t]) o b_hat[shared ? 0 : p][t]) for p < batch, n = 2^T.logn <= 4096,
// words of io_bits, on stream s (mac_dev.hpp k_mac).  hipErrorNotSupported for n > 4096,
// hipErrorInvalidValue for 32-bit words on a 64-bit modulus.
hipError_t launch_mac(const LaunchTables &T, const void *a, const void *b_hat, void *c,
                      size_t batch, uint32_t terms, int shared, int io_bits, hipStream_t s);
// The kernel launch_mac launches for (T, io_bits), as "k_mac<Arith32P,u32,u32,12>": the dry run of
// the launching statement itself (kernels_dev.hpp Emit)
hipError_t describe_mac(const LaunchTables &T, int io_bits, std::string *out);

}  // namespace nttmul
