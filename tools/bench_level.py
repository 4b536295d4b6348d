"""The view calls of lib/libnttmul_level.so against the dense calls on the pre-gathered operand, at
the same level of the chain, interleaved in one run per row, device-resident:

    python tools/bench_level.py [--rows 32:4096x16384:4x2x2,...] [--rots 4] [--rounds 7]
                                [--reps 0] [--warmup 2] [--mem-gib 16]
                                [--out profiles/level/bench.json]

A row is bits:n x batch:L x K x alpha, as tools/bench_lintrans.py's, with the same default rows.
Each row runs at two levels of its chain of L_top = L limbs: (L_top, L) = (L, L), the identity
view, and (L, L - 2), two rescales down.  The contexts are built on the first L primes; the key
b_hat [R][2][top_terms][L_top + K][n], the diagonals w_hat [R][L_top + K][n] and the
relinearisation key [2][top_terms][L_top + K][n] are made once for the top level; the dense side
reads their gathered copies, [..][terms][L + K][n], made before timing.  The batch of a row is
halved until its buffers fit --mem-gib; the row records the batch it ran.  Per level the timed
pairs are (device events around `reps` back-to-back calls, one synchronise per window)
  mac    nttmul_ksntt_mac_device           and nttmul_ksntt_mac_view_device        R rotations
  apply  nttmul_lintrans_apply_device      and nttmul_lintrans_apply_view_device   weights and c_0
  relin  nttmul_ctmul_relin_device         and nttmul_ctmul_relin_view_device      one pair
Dense and view run round-robin, `rounds` times, each round starting with the other one; a cell
reports the median, minimum and maximum window of each (ms per call), the dense side's own spread
((max - min) / median) and view over dense, and says whether the view is behind by more than that
spread.  Before timing, every view result is compared bit for bit with the dense one over the
whole batch.  --reps 0 picks 5 for rows whose a_hat holds at least 2^26 words and 50 below.

Every row also carries the figure the views exist for: the bytes of one rotation key
([2][terms][L + K][n]) a chain of L_top levels holds when every level has its dense copy, and
when the top-level key is stored once.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ",".join(f"{bits}:{shape}:{lka}" for shape in ("4096x16384", "65536x1024")
                        for bits in (32, 64) for lka in ("4x2x2", "12x4x4")) + \
    ",32:4096x64:4x2x2,64:4096x64:4x2x2"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 65536
COMPS = 2
DROP = 2                    # the second level of a row: L_top - DROP


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def rotation_list(n, rots):
    """The rotations of a rotate-and-sum step: one to R - 1 steps and the conjugation."""
    return [pow(5, i + 1, 2 * n) for i in range(rots - 1)] + [2 * n - 1]


def key_bytes(L_top, K, alpha, n, wb):
    """Bytes of one rotation key over a chain of L_top levels: a dense copy per level, and the
    top-level key alone."""
    per = lambda L: 2 * -(-L // alpha) * (L + K) * n * wb
    return {"dense_copy_per_level": sum(per(L) for L in range(1, L_top + 1)),
            "top_level_once": per(L_top)}


def row_polys(L_top, K, terms, rots):
    """Limb polynomials per batch entry of a row's buffers at the top level: a_hat, the mac's
    output, apply's and relin's outputs, each twice (view and dense), c0_hat, x_hat and y_hat."""
    M = L_top + K
    return terms * M + 2 * (rots * COMPS * M + 2 * COMPS * M) + 5 * L_top


def fit_batch(batch, polys, n, wb, limit):
    while batch > 1 and batch * polys * n * wb > limit:
        batch //= 2
    return batch


def random_words(torch, gen, moduli, lead, n, dtype):
    x = torch.empty((*lead, len(moduli), n), dtype=dtype, device="cuda")
    for l, m in enumerate(moduli):
        x[..., l, :] = torch.randint(0, m, (*lead, n), generator=gen, device="cuda",
                                     dtype=torch.int64).to(dtype)
    return x


def gather(top_operand, L, L_top, terms):
    """The dense operand of a level-L context (include/nttmul_level.h's top(m)), a copy."""
    K = top_operand.shape[-2] - L_top
    idx = list(range(L)) + list(range(L_top, L_top + K))
    if terms is not None:
        top_operand = top_operand[..., :terms, :, :]
    return top_operand[..., idx, :].contiguous()


def timed(torch, variants, rounds, reps, warmup):
    """{name: {median, min, max}} in ms per call, the variants interleaved round-robin."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    names = list(variants)
    ms = {k: [] for k in names}
    for r in range(rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                variants[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                "max": round(max(v), 5)} for k, v in ms.items()}


def cell(stat):
    spread = (stat["dense"]["max"] - stat["dense"]["min"]) / stat["dense"]["median"]
    ratio = stat["view"]["median"] / stat["dense"]["median"]
    return {"ms": stat, "view_over_dense": round(ratio, 3), "dense_spread": round(spread, 3),
            "behind_by_more_than_the_spread": bool(ratio - 1 > spread)}


def bench_level(torch, nttmul, bits, n, batch, L_top, L, K, alpha, primes, args):
    q_top, p = primes[:L_top], primes[L_top:]
    q = q_top[:L]
    ext, ext_top, M = q + p, q_top + p, L + K
    terms, top_terms, rots = -(-L // alpha), -(-L_top // alpha), args.rots
    view = (L_top, top_terms)
    kn = nttmul.NttLevelKeySwitch(n, q, p, min(alpha, L))
    lt, ct = nttmul.NttLevelLinTrans(n, q, p), nttmul.NttLevelCtMul(n, q, p)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L_top * 100 + L)
    reps = args.reps or (5 if batch * terms * M * n >= 1 << 26 else 50)
    kr = rotation_list(n, rots)

    a_hat = random_words(torch, gen, ext, (batch, terms), n, dtype)
    c0_hat = random_words(torch, gen, q, (batch,), n, dtype)
    x_hat = random_words(torch, gen, q, (batch, 1, 2), n, dtype)
    y_hat = random_words(torch, gen, q, (batch, 1, 2), n, dtype)
    key_top = random_words(torch, gen, ext_top, (rots, COMPS, top_terms), n, dtype)
    w_top = random_words(torch, gen, ext_top, (rots,), n, dtype)
    rk_top = random_words(torch, gen, ext_top, (2, top_terms), n, dtype)
    key, w, rk = gather(key_top, L, L_top, terms), gather(w_top, L, L_top, None), \
        gather(rk_top, L, L_top, terms)
    new = lambda *shape: torch.empty(shape, dtype=dtype, device="cuda")
    mac_out = {k: new(batch, rots, COMPS, M, n) for k in ("dense", "view")}
    lin_out = {k: new(batch, COMPS, M, n) for k in ("dense", "view")}
    rel_out = {k: new(batch, 2, M, n) for k in ("dense", "view")}

    def pair(dense, viewed):
        return {"dense": dense, "view": viewed}

    groups = {
        "mac": pair(
            lambda: kn.mac_device(mac_out["dense"], a_hat, key, kr, batch, terms, COMPS,
                                  stream=stream),
            lambda: kn.mac_device(mac_out["view"], a_hat, key_top, kr, batch, terms, COMPS,
                                  stream=stream, view=view)),
        "apply": pair(
            lambda: lt.apply_device(lin_out["dense"], a_hat, key, kr, batch, terms, COMPS,
                                    w_hat=w, c0_hat=c0_hat, stream=stream),
            lambda: lt.apply_device(lin_out["view"], a_hat, key_top, kr, batch, terms, COMPS,
                                    w_hat=w_top, c0_hat=c0_hat, stream=stream, view=view)),
        "relin": pair(
            lambda: ct.relin_device(rel_out["dense"], a_hat, rk, x_hat, y_hat, batch, 1, terms,
                                    stream=stream),
            lambda: ct.relin_device(rel_out["view"], a_hat, rk_top, x_hat, y_hat, batch, 1, terms,
                                    stream=stream, view=view)),
    }
    out = {"q_limbs": L, "terms": terms, "reps": reps, "cells": {}}
    for name, outs in (("mac", mac_out), ("apply", lin_out), ("relin", rel_out)):
        for fn in groups[name].values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(outs["view"], outs["dense"]), f"{name}: the view differs from the dense call"
        out["cells"][name] = cell(timed(torch, groups[name], args.rounds, reps, args.warmup))
    logn = n.bit_length() - 1
    out["kernels"] = {"mac": nttmul.level_kernel_name("mac", logn, bits, COMPS),
                      "apply": nttmul.level_kernel_name("lintrans", logn, bits, COMPS, True),
                      "relin": nttmul.level_kernel_name("relin", logn, bits)}
    for h in (kn, lt, ct):
        h.close()
    return out


def bench_row(torch, nttmul, bits, n, batch, L_top, K, alpha, args):
    if L_top - DROP < 1:
        raise ValueError(f"L = {L_top}: a row needs at least {DROP + 1} limbs of Q")
    primes = primes_below(nttmul, TOP[bits], L_top + K)
    wb = bits // 8
    asked = batch
    batch = fit_batch(batch, row_polys(L_top, K, -(-L_top // alpha), args.rots), n, wb,
                      args.mem_gib << 30)
    row = {"word_bits": bits, "n": n, "batch": batch, "batch_asked": asked, "top_q_limbs": L_top,
           "p_limbs": K, "digit_limbs": alpha, "top_terms": -(-L_top // alpha), "rots": args.rots,
           "comps": COMPS, "key_bytes_of_a_chain": key_bytes(L_top, K, alpha, n, wb), "levels": []}
    for L in (L_top, L_top - DROP):
        row["levels"].append(bench_level(torch, nttmul, bits, n, batch, L_top, L, K, alpha, primes,
                                         args))
        torch.cuda.empty_cache()
    return row


def parse_rows(text):
    rows = []
    for item in text.split(","):
        bits, shape, limbs = item.split(":")
        n, batch = (int(v) for v in shape.split("x"))
        L, K, alpha = (int(v) for v in limbs.split("x"))
        if int(bits) not in TOP:
            raise ValueError(f"word bits {bits}: 32 or 64")
        rows.append((int(bits), n, batch, L, K, alpha))
    return rows


def dump(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(obj) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed pairs")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:L x K x alpha, e.g. 32:4096x16384:4x2x2")
    ap.add_argument("--rots", type=int, default=4, help="rotations of mac and apply, 1 .. 16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mem-gib", type=int, default=16,
                    help="the batch of a row is halved until its buffers fit this many GiB")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
        if not 1 <= args.rots <= 16:
            raise ValueError("rotation counts are 1 .. 16")
    except ValueError as e:
        ap.error(f"--rows / --rots: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_level.py measures on a GPU; none is visible")
    line = {"bench": "level", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "mem_gib": args.mem_gib, "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, *row, args))
        torch.cuda.empty_cache()
        print(f"row {len(line['rows'])} of {len(rows)} done", file=sys.stderr, flush=True)
        if args.out:                       # the rows so far, should a later one be cut short
            dump(args.out, line)
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
