"""One launch over all limbs of an RNS basis (lib/libnttmul_rns.so, nttmul_rns_*_device) against
what a caller does today: L calls of the plain entry point on L single-modulus contexts over
limb-major [L][batch][n] copies, on one stream.  Device-resident, interleaved in one run:

    python tools/bench_rns.py [--shapes 4096x16384,4096x64,1024x1024] [--limbs 4] [--rounds 9]
                              [--reps 0] [--warmup 3] [--out profiles/rns/bench.json]

Per shape n x batch, with the first --limbs primes of the 32-bit basis, the timed sequences are
(device events around `reps` back-to-back calls, one synchronise per window):
  rns_multiply / rns_forward / rns_inverse / rns_mac_t4_shared     one nttmul_rns_*_device call
  plain_multiply / plain_forward / plain_inverse / plain_mac_t4_shared
                                 L calls of the plain entry point (the mac: nttmul_mac_ntt_device
                                 of lib/libnttmul_mac.so, which holds libnttmul.so's kernels bit
                                 for bit), one per limb
The eight run round-robin, `rounds` times, each round starting one variant later; the line reports
the median, minimum and maximum window of each (ms per operation over all limbs), per operation
the ratio rns / plain of the medians and the plain side's own spread (max - min) / median, and the
kernel hashes of the kernels involved.  Before timing, each pair is compared bit for bit.  --reps 0
picks 20 for shapes of at least 16384 limb polynomials and 200 below.  Prints one JSON line (and
writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

BASIS32 = (2013265921, 2147352577, 1073872897, 1073479681, 786433)   # 2 * 4096 | q - 1, q < 2^31
OPS = ("multiply", "forward", "inverse", "mac_t4_shared")
TERMS = 4


def bench_shape(torch, nttmul, n, batch, moduli, args):
    L, T, bits = len(moduli), TERMS, 32
    stream = torch.cuda.current_stream().cuda_stream
    rns = nttmul.RnsContext(n, moduli)
    plain = [nttmul.MacContext(n, q) for q in moduli]

    def buf(polys):
        return torch.empty(polys * n, dtype=torch.int32, device="cuda")

    # limb-major operands, filled per limb (canonical for its modulus): a, b [L][batch][n] for the
    # product and the transforms, at [L][batch][T][n] and the shared bh [L][T][n] for the mac
    a_lm, b_lm, c_lm = ([buf(batch) for _ in range(L)] for _ in range(3))
    at_lm, bt_lm, bh_lm = [buf(batch * T) for _ in range(L)], [buf(T) for _ in range(L)], \
        [buf(T) for _ in range(L)]
    scratch = buf(batch * T)
    for l, ctx in enumerate(plain):
        ctx.fill_random_device(a_lm[l], b_lm[l], 0, batch, bits, stream=stream)
        ctx.fill_random_device(at_lm[l], scratch, batch, batch * T, bits, stream=stream)
        ctx.fill_random_device(bt_lm[l], scratch, batch * (T + 1), T, bits, stream=stream)
        ctx.forward_device(bh_lm[l], bt_lm[l], T, bits, stream=stream)
    del scratch

    def interleave(parts, inner):
        """[L] arrays of [outer][inner words] -> one [outer][L][inner words] array."""
        return torch.stack([x.view(-1, inner) for x in parts], dim=1).contiguous().view(-1)

    a, b = interleave(a_lm, n), interleave(b_lm, n)              # [batch][L][n]
    at = interleave(at_lm, n)                                    # [batch * T][L][n]
    bh = interleave(bh_lm, n)                                    # [T][L][n]
    c = buf(batch * L)

    def plain_calls(op):
        for l, ctx in enumerate(plain):
            if op == "multiply":
                ctx.multiply_device(c_lm[l], a_lm[l], b_lm[l], batch, bits, stream=stream)
            elif op == "forward":
                ctx.forward_device(c_lm[l], a_lm[l], batch, bits, stream=stream)
            elif op == "inverse":
                ctx.inverse_device(c_lm[l], a_lm[l], batch, bits, stream=stream)
            else:
                ctx.mac_ntt_device(c_lm[l], at_lm[l], bh_lm[l], batch, T, bits, shared=True,
                                   stream=stream)

    def rns_call(op):
        if op == "multiply":
            rns.multiply_device(c, a, b, batch, stream=stream)
        elif op == "forward":
            rns.forward_device(c, a, batch, stream=stream)
        elif op == "inverse":
            rns.inverse_device(c, a, batch, stream=stream)
        else:
            rns.mac_ntt_device(c, at, bh, batch, T, shared=True, stream=stream)

    variants = {}
    for op in OPS:
        variants["rns_" + op] = lambda op=op: rns_call(op)
        variants["plain_" + op] = lambda op=op: plain_calls(op)

    for op in OPS:  # both sides compute the same thing, bit for bit
        rns_call(op)
        plain_calls(op)
        assert torch.equal(c, interleave(c_lm, n)), f"{op}: the limb launch and the L plain calls differ"

    reps = args.reps or (20 if batch * L >= 16384 else 200)
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    names = list(variants)
    ms = {k: [] for k in names}
    for r in range(args.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                variants[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)

    med = {k: statistics.median(v) for k, v in ms.items()}
    compare = {}
    for op in OPS:
        p = ms["plain_" + op]
        ratio, spread = med["rns_" + op] / med["plain_" + op], (max(p) - min(p)) / med["plain_" + op]
        compare[op] = {"rns/plain": round(ratio, 4), "plain_spread": round(spread, 4),
                       "within_spread": bool(ratio <= 1 + spread)}
    rns_hashes = nttmul.kernel_hashes(nttmul.RNS_LIB_PATH)
    mac_hashes = nttmul.kernel_hashes(nttmul.MAC_LIB_PATH)
    rns_keys = [rns.kernel_name(i) for i in range(4)]
    logn = n.bit_length() - 1
    plain_keys = [nttmul.dispatch_key(plain[0].kernel_name(bits, batch)),
                  f"k_xform<Arith32P,u32,u32,{logn},0,0>", f"k_xform<Arith32P,u32,u32,{logn},0,1>",
                  nttmul.dispatch_key(plain[0].mac_kernel_name(bits))]
    out = {
        "n": n, "batch": batch, "limbs": L, "limb_polynomials": batch * L, "reps": reps,
        "ms_per_op": {k: {"median": round(med[k], 5), "min": round(min(v), 5),
                          "max": round(max(v), 5)} for k, v in ms.items()},
        "compare": compare,
        "kernel_hashes": {"libnttmul_rns.so": {k: rns_hashes[k] for k in rns_keys},
                          "libnttmul_mac.so": {k: mac_hashes[k] for k in plain_keys}},
    }
    rns.close()
    for ctx in plain:
        ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--shapes", default="4096x16384,4096x64,1024x1024",
                    help="comma-separated n x batch (batch counts polynomials of L limbs)")
    ap.add_argument("--limbs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if not 1 <= args.limbs <= len(BASIS32):
        ap.error(f"--limbs must be 1 .. {len(BASIS32)}")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_rns.py measures on a GPU; none is visible")
    moduli = BASIS32[:args.limbs]
    line = {"bench": "rns", "device": torch.cuda.get_device_name(0), "moduli": list(moduli),
            "word_bits": 32, "terms": TERMS, "rounds": args.rounds, "warmup": args.warmup,
            "shapes": [bench_shape(torch, nttmul, n, batch, moduli, args) for n, batch in shapes]}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
