"""The weighted sum of rotations before ModDown (lib/libnttmul_lintrans.so) and the linear transform
built on it, against the key mac and the ModDown over every rotation they replace and against a
device-to-device copy, interleaved in one run per row, device-resident:

    python tools/bench_lintrans.py [--rows 32:4096x16384:4x2x2,...] [--rots 1,2,4,8] [--rounds 7]
                                   [--reps 0] [--warmup 2] [--mem-gib 48]
                                   [--lib slots=lib/ab/libnttmul_lintrans_slots.so,...]
                                   [--out profiles/lintrans/bench.json]
                                   [--ab-out profiles/lintrans/slicing_ab.json]

A row is bits:n x batch:L x K x alpha, as tools/bench_ksntt.py's, with the same default rows:
n = 4096 x 16,384 and n = 65536 x 1,024 in both word classes for (L, K, alpha) = (4, 2, 2) and
(12, 4, 4), and the thin shape n = 4096 x 64.  The batch of a row is halved until the row's
buffers for the largest R fit --mem-gib; the row records the batch it ran.  Per row and per R in
--rots, with comps = 2, terms = dnum, weights and c_0 on and the real rotation list (5^1 ..
5^(R-1) and the conjugation 2n - 1), the timed sequences are (device events around `reps`
back-to-back sequences, one synchronise per window):
  apply        one nttmul_lintrans_apply_device call (1 launch)
  apply_<name> the same call on each library of --lib (the other forms of k_lintrans: Makefile
               ab-lintrans), for the slicing A/B
  mac          one nttmul_ksntt_mac_device call at the same R (1 launch): strictly less work, no
               weights, no c_0, no sum, and R times as many words written
  copy         a device-to-device copy of up_hat's bytes
  chain        apply, then nttmul_mdntt_moddown_device over batch * 2 polynomials (1 + 2 launches,
               1 + 4 above n = 4096)
  chain_today  mac, then nttmul_mdntt_moddown_device over batch * R * 2 polynomials, without the
               weighted sum it would still owe: the comparison favours this side
The variants of a group run round-robin, `rounds` times, each round starting one variant later; the
line reports the median, minimum and maximum window of each (ms per sequence), the baseline's own
spread ((max - min) / median), the yardstick a lead has to exceed, and for apply the ratio of its
median to its bound, ((terms + comps) (L + K) + L) n w bytes per input at the rate the interleaved
copy reached (2 bytes moved per byte copied).  Before timing, apply's result on the first entries
of the batch (a partial last workgroup among them) is compared bit for bit with the composition of
nttmul_ksntt_mac_device calls, and every --lib result with apply's over the whole batch.  --reps 0
picks 5 for rows whose up_hat holds at least 2^26 words and 50 below.  Prints one JSON line (and
writes it to --out; --ab-out gets the apply columns alone)."""
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
CHECK_ENTRIES = 33          # verified against the composition: eight full workgroups and one entry


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
    """Limb polynomials per batch entry of a row's buffers at R = rots: x_hat and c0_hat, the
    raised digits and the copy's target, the mac's output and its ModDown's, apply's output twice
    (the library's and a --lib one's) and its ModDown's."""
    return 2 * L + 2 * dnum * M + rots * COMPS * (M + L) + 2 * COMPS * M + COMPS * L


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


def composition(torch, kn, a, b, w, c0, kr, q, p):
    """apply as nttmul_ksntt_mac_device calls on device-resident operands: the per-rotation mac,
    its weighted sum as a mac over the rotations with k = {1}; w_hat (P mod m_l) as a mac against
    a constant polynomial, the c_0 term padded with zero P limbs through the same two steps; the
    last addition mod m_l in int64 (every modulus is below 2^62)."""
    ext, L = q + p, len(q)
    batch, terms, M, n = a.shape
    rots, comps = b.shape[:2]
    new = lambda *shape: torch.empty(shape, dtype=a.dtype, device="cuda")
    m = new(batch, rots, comps, M, n)
    kn.mac_device(m, a, b, kr, batch, terms, comps)
    out = new(batch, comps, M, n)
    kn.mac_device(out, m.permute(0, 2, 1, 3, 4).contiguous(), w, (1,), batch * comps, rots, 1)
    pconst = torch.zeros((M, n), dtype=a.dtype, device="cuda")
    P = 1
    for v in p:
        P *= v
    for l, mod in enumerate(q):
        pconst[l] = P % mod
    wp = new(rots, M, n)
    kn.mac_device(wp, w, pconst, (1,), rots, 1, 1)
    pad = torch.zeros((batch, 1, M, n), dtype=a.dtype, device="cuda")
    pad[:, 0, :L] = c0
    z, zs = new(batch, rots, M, n), new(batch, M, n)
    kn.mac_device(z, pad, wp, kr, batch, 1, 1)
    kn.mac_device(zs, z, torch.ones_like(w), (1,), batch, rots, 1)
    torch.cuda.synchronize()
    for l, mod in enumerate(ext):
        s = out[:, 0, l].to(torch.int64) + zs[:, l].to(torch.int64)
        out[:, 0, l] = torch.where(s >= mod, s - mod, s).to(a.dtype)
    return out


def bench_row(torch, nttmul, bits, n, batch, L, K, alpha, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    ext, M, dnum, wb = q + p, L + K, -(-L // alpha), bits // 8
    rot_counts = sorted(args.rot_list)
    asked = batch
    batch = fit_batch(batch, L, M, n, dnum, rot_counts[-1], wb, args.mem_gib << 30)
    kn, md = nttmul.NttKeySwitch(n, q, p, alpha), nttmul.NttModDown(n, q, p)
    lt = nttmul.NttLinTrans(n, q, p)
    others = {name: nttmul.NttLinTrans(n, q, p, lib_path=path) for name, path in args.libs}
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)
    reps = args.reps or (5 if batch * dnum * M * n >= 1 << 26 else 50)

    x_hat = random_words(torch, gen, q, (batch,), n, dtype)
    c0_hat = random_words(torch, gen, q, (batch,), n, dtype)
    up_hat = torch.empty((batch, dnum, M, n), dtype=dtype, device="cuda")
    up_copy = torch.empty_like(up_hat)
    kn.modup_device(up_hat, x_hat, batch, stream=stream)
    c_new = torch.empty((batch, COMPS, M, n), dtype=dtype, device="cuda")
    c_other = torch.empty_like(c_new)
    out_new = torch.empty((batch, COMPS, L, n), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    row = {"word_bits": bits, "n": n, "batch": batch, "batch_asked": asked, "q_limbs": L,
           "p_limbs": K, "digit_limbs": alpha, "digits": dnum, "reps": reps, "comps": COMPS,
           "weights": True, "c0": True, "rots": []}
    hashes = nttmul.kernel_hashes(nttmul.LINTRANS_LIB_PATH)
    names = [lt.kernel_name(COMPS, True), kn.kernel_name("mac", COMPS)] + \
        md.kernel_name().split(" + ")
    row["kernel_hashes"] = {k: hashes[nttmul.dispatch_key(k)] for k in names}

    for rots in rot_counts:
        kr = rotation_list(n, rots)
        key_hat = random_words(torch, gen, ext, (rots, COMPS, dnum), n, dtype)
        w_hat = random_words(torch, gen, ext, (rots,), n, dtype)
        c_old = torch.empty((batch, rots, COMPS, M, n), dtype=dtype, device="cuda")
        out_old = torch.empty((batch, rots, COMPS, L, n), dtype=dtype, device="cuda")

        def apply_on(ctx, c):
            ctx.apply_device(c, up_hat, key_hat, kr, batch, dnum, COMPS, w_hat=w_hat,
                             c0_hat=c0_hat, stream=stream)

        def apply_new():
            apply_on(lt, c_new)

        def mac_today():
            kn.mac_device(c_old, up_hat, key_hat, kr, batch, dnum, COMPS, stream=stream)

        def chain_new():
            apply_new()
            md.moddown_device(out_new, c_new, batch * COMPS, stream=stream)

        def chain_today():
            mac_today()
            md.moddown_device(out_old, c_old, batch * rots * COMPS, stream=stream)

        apply_new()
        chk = min(batch, CHECK_ENTRIES)
        want = composition(torch, kn, up_hat[:chk], key_hat, w_hat, c0_hat[:chk], kr, q, p)
        torch.cuda.synchronize()
        assert torch.equal(c_new[:chk], want), "apply differs from the composition"
        del want
        variants = {"apply": apply_new}
        for name, ctx in others.items():
            apply_on(ctx, c_other)
            torch.cuda.synchronize()
            assert torch.equal(c_other, c_new), f"apply_{name} differs from apply"
            variants[f"apply_{name}"] = (lambda ctx=ctx: apply_on(ctx, c_other))
        variants.update(mac=mac_today, copy=lambda: up_copy.copy_(up_hat, non_blocking=True))
        st = timed(torch, variants, args.rounds, reps, args.warmup)
        st.update(timed(torch, {"chain": chain_new, "chain_today": chain_today}, args.rounds,
                        max(1, reps // 2), args.warmup))
        poly = batch * n * wb
        copy_tbps = 2 * dnum * M * poly / (st["copy"]["median"] * 1e-3) / 1e12
        nbytes = ((dnum + COMPS) * M + L) * poly
        bound = nbytes / (copy_tbps * 1e12) * 1e3
        ab = {k: round(st[k]["median"] / st["apply"]["median"], 3) for k in st
              if k.startswith("apply_")}
        row["rots"].append({
            "rots": rots, "ms": st, "copy_tbps": round(copy_tbps, 3),
            "apply": {**lead_of(st, "apply", "mac"), "bound_bytes": nbytes,
                      "bound_ms_at_copy_rate": round(bound, 5),
                      "median_over_bound": round(st["apply"]["median"] / bound, 3),
                      "mac_bound_bytes": (dnum + rots * COMPS) * M * poly,
                      "other_over_apply": ab},
            "chain": {**lead_of(st, "chain", "chain_today"),
                      "launches": {"new": 3 if n <= 4096 else 5, "today": 3 if n <= 4096 else 5},
                      "moddown_polys": {"new": batch * COMPS, "today": batch * rots * COMPS}}})
        del key_hat, w_hat, c_old, out_old
        torch.cuda.empty_cache()
    for h in (kn, md, lt, *others.values()):
        h.close()
    return row


def ab_view(line):
    """The apply columns alone: the slicing A/B."""
    keep = ("word_bits", "n", "batch", "q_limbs", "p_limbs", "digits", "reps")
    rows = []
    for row in line["rows"]:
        rows.append({**{k: row[k] for k in keep},
                     "rots": [{"rots": r["rots"],
                               "ms": {k: v for k, v in r["ms"].items() if k.startswith("apply")},
                               "other_over_apply": r["apply"]["other_over_apply"]}
                              for r in row["rots"]]})
    return {**{k: v for k, v in line.items() if k != "rows"}, "bench": "lintrans slicing A/B",
            "rows": rows}


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


def parse_libs(text):
    libs = []
    for item in filter(None, text.split(",")):
        name, path = item.split("=")
        path = path if os.path.isabs(path) else os.path.join(
            ROOT, "ntt-based-polynomial-multiplier-fpga_amd", path)
        if not os.path.exists(path):
            raise ValueError(f"{path} not built: make ab-lintrans")
        libs.append((name, path))
    return libs


def dump(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(obj) + "\n")


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
    ap.add_argument("--lib", default="",
                    help="comma-separated name=path of other builds of the library (relative to "
                         "the package directory), e.g. slots=lib/ab/libnttmul_lintrans_slots.so")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--ab-out", default=None, help="write the apply columns alone to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
        args.rot_list = [int(v) for v in args.rots.split(",")]
        if not args.rot_list or min(args.rot_list) < 1 or max(args.rot_list) > 16:
            raise ValueError("rotation counts are 1 .. 16")
        args.libs = parse_libs(args.lib)
    except ValueError as e:
        ap.error(f"--rows / --rots / --lib: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_lintrans.py measures on a GPU; none is visible")
    line = {"bench": "lintrans", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "mem_gib": args.mem_gib,
            "libs": [name for name, _ in args.libs], "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, *row, args))
        torch.cuda.empty_cache()
        print(f"row {len(line['rows'])} of {len(rows)} done", file=sys.stderr, flush=True)
        if args.out:                       # the rows so far, should a later one be cut short
            dump(args.out, line)
        if args.ab_out:
            dump(args.ab_out, ab_view(line))
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
