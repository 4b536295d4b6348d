"""ModUp and the key mac on NTT-domain limbs (lib/libnttmul_ksntt.so) and the NTT-domain key switch
built from them, against what they replace and against a device-to-device copy of the output's
bytes, interleaved in one run per row, device-resident:

    python tools/bench_ksntt.py [--rows 32:4096x16384:4x2x2,...] [--rots 1,2,4,8] [--rounds 7]
                                [--reps 0] [--warmup 2] [--mem-gib 48]
                                [--out profiles/ksntt/bench.json]

A row is bits:n x batch:L x K x alpha, as tools/bench_hoist.py's, with the same default rows:
n = 4096 x 16,384 and n = 65536 x 1,024 in both word classes for (L, K, alpha) = (4, 2, 2) and
(12, 4, 4), and the thin shape n = 4096 x 64.  The batch of a row is halved until the row's
buffers for the largest R fit --mem-gib; the row records the batch it ran.  Per row the timed
sequences are (device events around `reps` back-to-back sequences, one synchronise per window):
  modup        one nttmul_ksntt_modup_device call (2 launches up to n = 4096, 4 above)
  modup_today  inverse over the L limbs, nttmul_ks_modup_device, forward over batch * dnum
               polynomials of L + K limbs (3 launches, 5 above)
  modup_copy   a device-to-device copy of up_hat's bytes
and per R in --rots, with comps = 2, terms = dnum and the real rotation list (5^1 .. 5^(R-1) and
the conjugation 2n - 1):
  mac          one nttmul_ksntt_mac_device call (1 launch)
  mac_today    hoist_ntt_device, then forward over batch * R * 2 polynomials (2 launches, 4 above)
  mac_copy     a device-to-device copy of c_hat's bytes
  chain        modup, mac, nttmul_mdntt_moddown_device (5 launches, 9 above)
  chain_today  inverse, ks_modup, forward, hoist_ntt, ks_moddown, forward (6 launches, 10 above)
The baselines are the compositions on the same commit in the same run.  The variants of a group
run round-robin, `rounds` times, each round starting one variant later; the line reports the
median, minimum and maximum window of each (ms per sequence), the baseline's own spread
((max - min) / median), the yardstick a lead has to exceed, and for mac the ratio of its median to
its bound, (terms + R comps) (L + K) n w bytes at the rate the interleaved copy reached (2 bytes
moved per byte copied).  Before timing every new result is compared bit for bit with its
baseline's.  --reps 0 picks 5 for rows whose up_hat holds at least 2^26 words and 50 below.  Prints one
JSON line (and writes it to --out)."""
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


def row_polys(L, M, dnum, rots):
    """Limb polynomials per batch entry of a row's buffers at R = rots: x_hat and its coefficient
    form, the raised digits three times (coefficients, today's transform, modup's), the mac's
    output three times, ModDown's three times."""
    return 2 * L + 3 * dnum * M + 3 * rots * COMPS * M + 3 * rots * COMPS * L


def fit_batch(batch, L, M, n, dnum, rots, wb, limit):
    while batch > 1 and batch * row_polys(L, M, dnum, rots) * n * wb > limit:
        batch //= 2
    return batch


def random_words(torch, gen, moduli, lead, n, dtype):
    x = torch.empty((*lead, len(moduli), n), dtype=dtype, device="cuda")
    for l, m in enumerate(moduli):
        x[..., l, :] = torch.randint(0, m, (*lead, n), generator=gen, device="cuda",
                                     dtype=torch.int64).to(dtype)
    return x


def timed(torch, variants, rounds, reps, warmup):
    """{name: {median, min, max}} in ms per sequence, the variants interleaved round-robin."""
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


def lead_of(stat, new, old):
    spread = (stat[old]["max"] - stat[old]["min"]) / stat[old]["median"]
    lead = stat[old]["median"] / stat[new]["median"]
    return {"today_over_new": round(lead, 3), "today_spread": round(spread, 3),
            "ahead_by_more_than_the_spread": bool(lead - 1 > spread)}


def bench_row(torch, nttmul, bits, n, batch, L, K, alpha, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    ext, M, dnum, wb = q + p, L + K, -(-L // alpha), bits // 8
    rot_counts = sorted(args.rot_list)
    asked = batch
    batch = fit_batch(batch, L, M, n, dnum, rot_counts[-1], wb, args.mem_gib << 30)
    Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    kn, md = nttmul.NttKeySwitch(n, q, p, alpha), nttmul.NttModDown(n, q, p)
    big, low, ks = Ctx(n, ext), Ctx(n, q), nttmul.KeySwitchBasis(n, q, p, alpha)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)
    reps = args.reps or (5 if batch * dnum * M * n >= 1 << 26 else 50)

    x_hat = random_words(torch, gen, q, (batch,), n, dtype)
    coef = torch.empty_like(x_hat)
    up_new = torch.empty((batch, dnum, M, n), dtype=dtype, device="cuda")
    up, up_hat = torch.empty_like(up_new), torch.empty_like(up_new)

    def modup_today():
        low.inverse_device(coef, x_hat, batch, stream=stream)
        ks.modup_device(up, coef, batch, stream=stream)
        big.forward_device(up_hat, up, batch * dnum, stream=stream)

    def modup_new():
        kn.modup_device(up_new, x_hat, batch, stream=stream)

    modup_new()
    modup_today()
    torch.cuda.synchronize()
    assert torch.equal(up_new, up_hat), "modup differs from the composition"
    stat = timed(torch, {"modup": modup_new, "modup_today": modup_today,
                         "modup_copy": lambda: up.copy_(up_hat, non_blocking=True)},
                 args.rounds, reps, args.warmup)
    row = {"word_bits": bits, "n": n, "batch": batch, "batch_asked": asked, "q_limbs": L,
           "p_limbs": K, "digit_limbs": alpha, "digits": dnum, "reps": reps,
           "modup": {"ms": stat, **lead_of(stat, "modup", "modup_today"),
                     "launches": {"new": 2 if n <= 4096 else 4, "today": 3 if n <= 4096 else 5},
                     "transforms": {"new": dnum * M, "today": L + dnum * M}},
           "rots": []}
    hashes = nttmul.kernel_hashes(nttmul.KSNTT_LIB_PATH)
    names = kn.kernel_name("modup").split(" + ") + [kn.kernel_name("mac", COMPS)]
    row["kernel_hashes"] = {k: hashes[nttmul.dispatch_key(k)] for k in names}

    for rots in rot_counts:
        kr = rotation_list(n, rots)
        key_hat = random_words(torch, gen, ext, (rots, COMPS, dnum), n, dtype)
        c_new = torch.empty((batch, rots, COMPS, M, n), dtype=dtype, device="cuda")
        mid, mid_hat = torch.empty_like(c_new), torch.empty_like(c_new)
        out_new = torch.empty((batch, rots, COMPS, L, n), dtype=dtype, device="cuda")
        down, down_hat = torch.empty_like(out_new), torch.empty_like(out_new)
        units = batch * rots * COMPS

        def mac_today():
            big.hoist_ntt_device(mid, up_hat, key_hat, kr, batch, dnum, COMPS, stream=stream)
            big.forward_device(mid_hat, mid, units, stream=stream)

        def mac_new():
            kn.mac_device(c_new, up_hat, key_hat, kr, batch, dnum, COMPS, stream=stream)

        def chain_today():
            modup_today()
            big.hoist_ntt_device(mid, up_hat, key_hat, kr, batch, dnum, COMPS, stream=stream)
            ks.moddown_device(down, mid, units, stream=stream)
            low.forward_device(down_hat, down, units, stream=stream)

        def chain_new():
            modup_new()
            mac_new()
            md.moddown_device(out_new, c_new, units, stream=stream)

        mac_new()
        mac_today()
        torch.cuda.synchronize()
        assert torch.equal(c_new, mid_hat), "mac differs from the composition"
        chain_new()
        chain_today()
        torch.cuda.synchronize()
        assert torch.equal(out_new, down_hat), "the chain differs from the composition"
        st = timed(torch, {"mac": mac_new, "mac_today": mac_today,
                           "mac_copy": lambda: mid.copy_(mid_hat, non_blocking=True)},
                   args.rounds, reps, args.warmup)
        st.update(timed(torch, {"chain": chain_new, "chain_today": chain_today}, args.rounds,
                        max(1, reps // 2), args.warmup))
        poly = batch * n * wb
        copy_tbps = 2 * rots * COMPS * M * poly / (st["mac_copy"]["median"] * 1e-3) / 1e12
        nbytes = (dnum + rots * COMPS) * M * poly
        bound = nbytes / (copy_tbps * 1e12) * 1e3
        row["rots"].append({
            "rots": rots, "ms": st, "copy_tbps": round(copy_tbps, 3),
            "mac": {**lead_of(st, "mac", "mac_today"), "bound_bytes": nbytes,
                    "bound_ms_at_copy_rate": round(bound, 5),
                    "median_over_bound": round(st["mac"]["median"] / bound, 3),
                    "launches": {"new": 1, "today": 2 if n <= 4096 else 4}},
            "chain": {**lead_of(st, "chain", "chain_today"),
                      "launches": {"new": 5 if n <= 4096 else 9, "today": 6 if n <= 4096 else 10},
                      "transforms": {"new": dnum * M + COMPS * rots * M,
                                     "today": L + dnum * M + COMPS * rots * M + COMPS * rots * L}}})
        del key_hat, c_new, mid, mid_hat, out_new, down, down_hat
        torch.cuda.empty_cache()
    for h in (kn, md, big, low, ks):
        h.close()
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:L x K x alpha, e.g. 32:4096x16384:4x2x2")
    ap.add_argument("--rots", default="1,2,4,8", help="comma-separated rotation counts, 1 .. 16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="sequences per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mem-gib", type=int, default=48,
                    help="the batch of a row is halved until its buffers fit this many GiB")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
        args.rot_list = [int(v) for v in args.rots.split(",")]
        if not args.rot_list or min(args.rot_list) < 1 or max(args.rot_list) > 16:
            raise ValueError("rotation counts are 1 .. 16")
    except ValueError as e:
        ap.error(f"--rows / --rots: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_ksntt.py measures on a GPU; none is visible")
    line = {"bench": "ksntt", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "mem_gib": args.mem_gib, "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, *row, args))
        torch.cuda.empty_cache()
        print(f"row {len(line['rows'])} of {len(rows)} done", file=sys.stderr, flush=True)
        if args.out:                       # the rows so far, should a later one be cut short
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
