/*
 * nttmul_diag.h — the diagnostic build lib/libnttmul_diag.so (not libnttmul.so).
 *
 * Same C ABI and the same product kernels as include/nttmul.h, built with NTTMUL_CLOCK_STAMPS:
 * thread 0 of every k_rows workgroup (the fused product at n <= 4096, the row pass above)
 * stamps s_memtime and s_memrealtime at entry and after issuing its stores, so a caller can read
 * the shader clock the product kernel actually held (MI355X_MICROARCH.md 'DVFS give-back' item 6)
 * — bench.py puts it beside the VALU issue bound.  The stamps go to a buffer of their own; no
 * output depends on them.  The production library executes no stamp.
 *
 * The build also holds the failure points of the resident device server's host side and a
 * read-out of its state (nttmul_diag_server_failpoint, nttmul_diag_server_state below), for the
 * tests of the server's failure and retry paths (tests/test_gpu_server_failures.py).  The
 * production libraries hold neither the symbols nor a branch for them.
 */
#ifndef NTTMUL_DIAG_H
#define NTTMUL_DIAG_H

#include "nttmul.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The last k_rows launch's stamps of workgroups 0 .. blocks - 1 (at most 65536), four uint64 per
 * workgroup: entry s_memtime, entry s_memrealtime, end s_memtime, end s_memrealtime.  The
 * workgroup's clock is (end_t - entry_t) / (end_r - entry_r) x 100 MHz.  Call after the launch
 * has completed. */
int nttmul_diag_clock_stamps(uint64_t *dst, size_t blocks);

/* The resident device server's timeline of ctx's last host product served through it
 * (nttmul_last_host_path == 3; params.small_server): dst[0..3] = s_memrealtime (100 MHz) when
 * the kernel saw the request, had a and b loaded, had the product computed, had c stored and
 * released; dst[4], dst[5] = s_memtime (shader clock) around the product; dst[6] = host
 * nanoseconds from posting the request to seeing it done.  NTTMUL_EINVAL if the last call did not
 * go through the server. */
int nttmul_diag_server_stamps(const nttmul_ctx *ctx, uint64_t *dst);

/* Failure points of the resident device server's host side (csrc/nttmul.cpp run_server,
 * server_alloc, server_launch), for tests of its failure and retry paths.  A site names one
 * runtime call; an armed site lets `skip` further passes through and then, once, does NOT make
 * that call and takes hip_error (a hipError_t other than hipSuccess) as its result, so the
 * injected error runs through the library's own error text, failure counter and cool-down.
 * Nothing is injected on the device: a failure replaces a host call that is then not made. */
enum {
  NTTMUL_DIAG_SITE_BOX_ALLOC = 0,       /* server_alloc: hipHostMalloc of the result half */
  NTTMUL_DIAG_SITE_BOX_MAP = 1,         /* server_alloc: hipHostGetDevicePointer of it */
  NTTMUL_DIAG_SITE_STREAM = 2,          /* server_alloc: hipStreamCreateWithFlags */
  NTTMUL_DIAG_SITE_REQ_ALLOC = 3,       /* server_alloc: hipHostMalloc of the request half (only
                                           where it is not in fine-grained device memory) */
  NTTMUL_DIAG_SITE_REQ_MAP = 4,         /* server_alloc: hipHostGetDevicePointer of it (likewise) */
  NTTMUL_DIAG_SITE_LAUNCH = 5,          /* server_launch: the launch of the resident kernel */
  /* No error: the host sleeps three times the kernel's idle time (3 ms) just before it posts the
   * request, so the kernel has left through its idle exit while the host still takes it as
   * running, and the request is answered by the relaunch inside the host's spin loop.
   * hip_error is ignored. */
  NTTMUL_DIAG_SITE_STALL_BEFORE_GO = 6,
  NTTMUL_DIAG_SITE_COUNT = 7
};

/* Arm `site` of ctx (re-arming replaces; several sites may be armed at once).  NTTMUL_EINVAL
 * for a null context, an unknown site, or hipSuccess at a site that injects an error.  From the
 * thread that makes ctx's calls. */
int nttmul_diag_server_failpoint(nttmul_ctx *ctx, int site, int hip_error, unsigned skip);

/* The server's host-side state, read without a launch or any other runtime call.  The invariant
 * the library keeps: whenever no request is in flight, go == served (the resident kernel serves
 * whatever go word differs from the one it started from), and neither mailbox half is ever
 * split, i.e. held as a host pointer without its device pointer. */
typedef struct nttmul_diag_server_state_t {
  uint32_t go, done;        /* the go word as last posted; the result half's done word (both 0
                               before the mailbox exists) */
  uint32_t served, seq;     /* last go word answered; sequence number of the last go word posted */
  int32_t running;          /* the host takes the kernel as resident */
  uint32_t cooldown;        /* eligible calls left on the launch path before the next try */
  uint32_t failures;        /* as nttmul_server_status */
  int32_t small_server;     /* 0 automatic, -1 launch path for good */
  int32_t box_pair, req_pair; /* host and device pointer of each half: 2 both set, 0 both null,
                                 1 split */
  int32_t req_in_vram;      /* the request half lies in fine-grained device memory */
  uint32_t launches;        /* launches of the resident kernel that succeeded, */
  uint32_t spin_relaunches; /* ... those of them made inside the spin loop, */
  uint32_t stops;           /* and stop requests posted (server_stop) */
} nttmul_diag_server_state_t;
int nttmul_diag_server_state(const nttmul_ctx *ctx, nttmul_diag_server_state_t *out);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_DIAG_H */
