"""The limb launches of lib/libnttmul_rnsmp.so (nttmul_rnsmp_*_device, 4096 < n <= 65536) against
what a caller does today: L calls of the plain entry point on L single-modulus contexts of
lib/libnttmul.so over limb-major [L][batch][n] copies, on one stream.  Device-resident,
interleaved in one run:

    python tools/bench_rnsmp.py [--shapes 16384x4096,65536x1024,16384x16,65536x4] [--limbs 4]
                                [--words 32,64] [--rounds 9] [--reps 0] [--warmup 2]
                                [--scratch-mb 0] [--out profiles/rnsmp/bench.json]

Per word class and shape n x batch, with the first --limbs primes of the class's basis, the timed
sequences are (device events around `reps` back-to-back sequences, one synchronise per window):
  rnsmp_multiply / rnsmp_forward / rnsmp_inverse      one nttmul_rnsmp_*_device call: 3, 2, 2 launches
  rnsmp_mac_t4_shared                                 one nttmul_rnsmp_mac_ntt_device call: 3 launches
  plain_multiply / plain_forward / plain_inverse      L calls of the plain entry point: 3 L, 2 L, 2 L
                                                      launches
  plain_mac_t4_shared_no_adds   The plain ABI has no multiply-accumulate above n = 4096 and no
                                addition at all.  This is the sequence a caller can run today,
                                WITHOUT the additions it would still have to write: T L forward
                                calls, T L pointwise calls (against b_hat tiled over the batch
                                beforehand: the plain pointwise has no shared operand), L inverse
                                calls.  It computes less than the mac does.
The eight run round-robin, `rounds` times, each round starting one variant later; the line reports
the median, minimum and maximum window of each (ms per operation over all limbs), per operation
the ratio rnsmp / plain of the medians and the plain side's own spread (max - min) / median, and
the kernel hashes of the limb kernels.  Before timing, each pair is compared bit for bit (the mac
against the plain sequence with the additions done in torch).

Both sides keep the library's default scratch_mb (512 MiB per scratch buffer and context), so at a
fat shape the limb context runs sub-batches of 1 / L of the batch where each plain context takes
its limb in one pass; --scratch-mb sets the limb context's (512 L gives it one pass too: measured
slower for 64-bit words at n = 65536).  --reps 0 picks 5 for shapes of at least
2^26 words per operand and 100 below.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

# 2 * 65536 | q - 1, so each basis serves every n
BASES = {32: (2013265921, 2147352577, 1073872897, 1073479681, 786433),
         64: (4611686018425815041, 2305843009211596801, 1152921504606584833, 576460752300015617)}
OPS = ("multiply", "forward", "inverse", "mac_t4_shared")
PLAIN = {"multiply": "plain_multiply", "forward": "plain_forward", "inverse": "plain_inverse",
         "mac_t4_shared": "plain_mac_t4_shared_no_adds"}
TERMS = 4


def bench_shape(torch, nttmul, n, batch, moduli, bits, args):
    L, T = len(moduli), TERMS
    stream = torch.cuda.current_stream().cuda_stream
    tdt = torch.int32 if bits == 32 else torch.int64
    mp = nttmul.RnsMpContext(n, moduli, scratch_mb=args.scratch_mb)
    plain = [nttmul.Context(n, q) for q in moduli]

    def buf(polys):
        return torch.empty(polys * n, dtype=tdt, device="cuda")

    # limb-major operands, filled per limb (canonical for its modulus): a, b, c [L][batch][n]; the
    # mac's a as [L][T][batch][n] (one plain forward call per (limb, term)), b_hat [L][T][n] and
    # its copy tiled over the batch [L][T][batch][n] for the plain pointwise
    a_lm, b_lm, c_lm = ([buf(batch) for _ in range(L)] for _ in range(3))
    at_lm = [[buf(batch) for _ in range(T)] for _ in range(L)]
    tmp_lm = [[buf(batch) for _ in range(T)] for _ in range(L)]
    bh_lm = [buf(T) for _ in range(L)]
    junk = buf(max(batch, T))
    for l, ctx in enumerate(plain):
        ctx.fill_random_device(a_lm[l], b_lm[l], 0, batch, bits, stream=stream)
        for t in range(T):
            ctx.fill_random_device(at_lm[l][t], junk, batch * (t + 1), batch, bits, stream=stream)
        ctx.fill_random_device(junk, bh_lm[l], batch * (T + 1), T, bits, stream=stream)
        ctx.forward_device(bh_lm[l], bh_lm[l], T, bits, stream=stream)
    del junk
    bht_lm = [[bh_lm[l].view(T, n)[t].expand(batch, n).contiguous().view(-1) for t in range(T)]
              for l in range(L)]

    def interleave(parts):
        """[L] arrays of [outer][n] -> one [outer][L][n] array."""
        return torch.stack([x.view(-1, n) for x in parts], dim=1).contiguous().view(-1)

    a, b = interleave(a_lm), interleave(b_lm)                                    # [batch][L][n]
    at = torch.stack([torch.stack([at_lm[l][t].view(batch, n) for l in range(L)], dim=1)
                      for t in range(T)], dim=1).contiguous().view(-1)           # [batch][T][L][n]
    bh = interleave(bh_lm)                                                       # [T][L][n]
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
                for t in range(T):
                    ctx.forward_device(tmp_lm[l][t], at_lm[l][t], batch, bits, stream=stream)
                for t in range(T):
                    ctx.pointwise_device(tmp_lm[l][t], tmp_lm[l][t], bht_lm[l][t], batch, bits,
                                         stream=stream)
                ctx.inverse_device(c_lm[l], tmp_lm[l][0], batch, bits, stream=stream)

    def mp_call(op):
        if op == "multiply":
            mp.multiply_device(c, a, b, batch, stream=stream)
        elif op == "forward":
            mp.forward_device(c, a, batch, stream=stream)
        elif op == "inverse":
            mp.inverse_device(c, a, batch, stream=stream)
        else:
            mp.mac_ntt_device(c, at, bh, batch, T, shared=True, stream=stream)

    for op in OPS:  # both sides compute the same thing, bit for bit
        mp_call(op)
        plain_calls(op)
        if op == "mac_t4_shared":  # the additions the plain sequence leaves out, then its inverse
            for l, ctx in enumerate(plain):
                acc = tmp_lm[l][0].to(torch.int64)
                for t in range(1, T):
                    acc = acc + tmp_lm[l][t]           # canonical words: < 2 q < 2^63
                    acc = torch.where(acc >= moduli[l], acc - moduli[l], acc)
                ctx.inverse_device(c_lm[l], acc.to(tdt), batch, bits, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(c, interleave(c_lm)), f"{op}: the limb launches and the plain calls differ"

    variants = {}
    for op in OPS:
        variants["rnsmp_" + op] = lambda op=op: mp_call(op)
        variants[PLAIN[op]] = lambda op=op: plain_calls(op)

    reps = args.reps or (5 if batch * L * n >= (1 << 26) else 100)
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
        p = ms[PLAIN[op]]
        ratio = med["rnsmp_" + op] / med[PLAIN[op]]
        spread = (max(p) - min(p)) / med[PLAIN[op]]
        compare[op] = {"rnsmp/plain": round(ratio, 4), "plain_spread": round(spread, 4),
                       "within_spread": bool(ratio <= 1 + spread)}
    hashes = nttmul.kernel_hashes(nttmul.RNSMP_LIB_PATH)
    keys = sorted({k for i in range(4) for k in mp.kernel_name(i).split(" + ")})
    out = {
        "n": n, "batch": batch, "limbs": L, "limb_polynomials": batch * L, "reps": reps,
        "launches": {"rnsmp": {"multiply": 3, "forward": 2, "inverse": 2, "mac_t4_shared": 3},
                     "plain": {"multiply": 3 * L, "forward": 2 * L, "inverse": 2 * L,
                               "mac_t4_shared_no_adds": (2 * T + T + 2) * L}},
        "ms_per_op": {k: {"median": round(med[k], 5), "min": round(min(v), 5),
                          "max": round(max(v), 5)} for k, v in ms.items()},
        "compare": compare,
        "plain_product_kernels": plain[0].kernel_name(bits, batch),
        "kernel_hashes": {"libnttmul_rnsmp.so": {k: hashes[k] for k in keys}},
    }
    print(f"u{bits} {n} x {batch} x {L}: " + ", ".join(
        f"{op} {compare[op]['rnsmp/plain']}" for op in OPS), file=sys.stderr, flush=True)
    mp.close()
    for ctx in plain:
        ctx.close()
    del a, b, c, at, bh, a_lm, b_lm, c_lm, at_lm, tmp_lm, bh_lm, bht_lm
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--shapes", default="16384x4096,65536x1024,16384x16,65536x4",
                    help="comma-separated n x batch (batch counts polynomials of L limbs)")
    ap.add_argument("--limbs", type=int, default=4)
    ap.add_argument("--words", default="32,64", help="word classes, comma-separated")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=0, help="sequences per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scratch-mb", type=int, default=0,
                    help="the limb context's scratch_mb (0: the library default, 512)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    words = [int(w) for w in args.words.split(",")]
    if any(w not in BASES for w in words):
        ap.error("--words takes 32 and 64")
    if not 1 <= args.limbs <= min(len(BASES[w]) for w in words):
        ap.error("--limbs must be 1 .. 4")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnsmp.py measures on a GPU; none is visible")
    classes = []
    for bits in words:
        moduli = BASES[bits][:args.limbs]
        classes.append({"word_bits": bits, "moduli": list(moduli),
                        "shapes": [bench_shape(torch, nttmul, n, batch, moduli, bits, args)
                                   for n, batch in shapes]})
    line = {"bench": "rnsmp", "device": torch.cuda.get_device_name(0), "terms": TERMS,
            "rounds": args.rounds, "warmup": args.warmup,
            "scratch_mb": args.scratch_mb or 512, "classes": classes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
