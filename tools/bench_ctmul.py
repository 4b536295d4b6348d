"""The ciphertext product on NTT-domain limbs (lib/libnttmul_ctmul.so) against a device-to-device
copy, against the key mac it extends, and the whole multiplication against separate chains,
interleaved in one run per row, device-resident:

    python tools/bench_ctmul.py [--rows 32:4096x16384:4x2x2,...] [--pairs 1,4] [--rounds 7]
                                [--reps 0] [--warmup 2] [--mem-gib 48]
                                [--lib v2=lib/ab/libnttmul_ctmul_v2.so,...]
                                [--out profiles/ctmul/bench.json]

A row is bits:n x batch:L x K x alpha, as tools/bench_lintrans.py's, with the same default rows:
n = 4096 x 16,384 and n = 65536 x 1,024 in both word classes for (L, K, alpha) = (4, 2, 2) and
(12, 4, 4), and the thin shape n = 4096 x 64.  The batch of a row is halved until the row's
buffers for the largest `pairs` fit --mem-gib; the row records the batch it ran.  Per row and per
`pairs`, with terms = dnum, the timed sequences are (device events around `reps` back-to-back
sequences, one synchronise per window):
  high        one nttmul_ctmul_high_device call (1 launch)
  high_copy   a device-to-device copy moving high's bytes, (2 pairs + 1) L n w per entry
  relin       one nttmul_ctmul_relin_device call (1 launch)
  relin_<name> the same call on each library of --lib (another form of k_ctmul_relin: Makefile
              ab-ctmul), compared bit for bit with relin's result over the whole batch first
  apply       nttmul_lintrans_apply_device with k = {1}, no weights, no c_0, at the same terms
              (1 launch): strictly less work, no tensor terms
  relin_copy  a device-to-device copy moving relin's bytes, ((terms + 2)(L + K) + 4 pairs L) n w
  xy_copy     a device-to-device copy moving the 4 pairs L limb polynomials relin reads beyond
              apply
  chain       high, nttmul_ksntt_modup_device, relin, nttmul_mdntt_moddown_device over batch * 2
              polynomials (1 + 2 + 1 + 2 launches, 1 + 4 + 1 + 4 above n = 4096)
  chain_each  the pairs = 1 chain, `pairs` times: what a dot product costs without lazy
              relinearisation (without the additions it would still owe)
The variants of a group run round-robin, `rounds` times, each round starting one variant later; the
line reports the median, minimum and maximum window of each (ms per sequence), the other side's
own spread ((max - min) / median), the yardstick a lead has to exceed, and whether relin costs more
than apply plus xy_copy.  A copy of B bytes moves 2 B; a kernel's byte bound is its bytes at the
rate the interleaved copy of the same bytes reached.  Before timing, high's and relin's results on
the first entries of the batch (a partial last workgroup among them) are compared bit for bit with
the composition of existing calls.  --reps 0 picks 5 for rows whose up_hat holds at least 2^26
words and 50 below.  Prints one JSON line (and writes it to --out)."""
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
CHECK_ENTRIES = 33          # verified against the composition: eight full workgroups and one entry


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def row_polys(L, M, dnum, pairs):
    """Limb polynomials per batch entry of a row's buffers: x_hat and y_hat, d2_hat, up_hat,
    c_hat, the ModDown's output, and the largest copy's source and target."""
    return 4 * pairs * L + L + dnum * M + 2 * M + 2 * L + 2 * ((dnum + 2) * M + 4 * pairs * L)


def fit_batch(batch, L, M, n, dnum, pairs, wb, limit):
    while batch > 1 and batch * row_polys(L, M, dnum, pairs) * n * wb > limit:
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


def ratio_of(stat, new, old):
    """old / new with old's own spread: new leads when the ratio exceeds 1 by more than it."""
    spread = (stat[old]["max"] - stat[old]["min"]) / stat[old]["median"]
    lead = stat[old]["median"] / stat[new]["median"]
    return {"other_over_new": round(lead, 3), "other_spread": round(spread, 3),
            "ahead_by_more_than_the_spread": bool(lead - 1 > spread)}


def addmod(torch, x, y, m):
    s = x.to(torch.int64) + y.to(torch.int64)
    return torch.where(s >= m, s - m, s).to(x.dtype)


def composition(torch, kn, plain, up, key, x, y, q, p, bits):
    """(d2_hat, c_hat) from existing calls on device-resident operands: nttmul_ksntt_mac_device
    with k = {1} for the key sum, the plain contexts' pointwise products for the tensor terms and
    the factor P mod q_l, additions mod q_l in int64 (every modulus is below 2^62)."""
    batch, terms, M, n = up.shape
    pairs, L = x.shape[1], len(q)
    c = torch.empty((batch, 1, 2, M, n), dtype=up.dtype, device="cuda")
    kn.mac_device(c, up, key, (1,), batch, terms, 2)
    c = c[:, 0]
    d2 = torch.empty((batch, L, n), dtype=up.dtype, device="cuda")
    P = 1
    for v in p:
        P *= v

    def product(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        ctx.pointwise_device(out, a, b, a.numel() // n, bits)
        torch.cuda.synchronize()
        return out

    def over_pairs(t, m):
        acc = t[:, 0]
        for s in range(1, pairs):
            acc = addmod(torch, acc, t[:, s], m)
        return acc

    for l, (ctx, m) in enumerate(zip(plain, q)):
        x0, x1, y0, y1 = x[:, :, 0, l], x[:, :, 1, l], y[:, :, 0, l], y[:, :, 1, l]
        e0 = over_pairs(product(ctx, x0, y0), m)
        e1 = addmod(torch, over_pairs(product(ctx, x0, y1), m),
                    over_pairs(product(ctx, x1, y0), m), m)
        d2[:, l] = over_pairs(product(ctx, x1, y1), m)
        const = torch.full((batch, n), P % m, dtype=torch.int64, device="cuda").to(up.dtype)
        for i, e in enumerate((e0, e1)):
            c[:, i, l] = addmod(torch, c[:, i, l], product(ctx, e, const), m)
    return d2, c


def bench_row(torch, nttmul, bits, n, batch, L, K, alpha, args):
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    ext, M, dnum, wb = q + p, L + K, -(-L // alpha), bits // 8
    pair_counts = sorted(args.pair_list)
    asked = batch
    batch = fit_batch(batch, L, M, n, dnum, pair_counts[-1], wb, args.mem_gib << 30)
    kn, md = nttmul.NttKeySwitch(n, q, p, alpha), nttmul.NttModDown(n, q, p)
    ct, lt = nttmul.NttCtMul(n, q, p), nttmul.NttLinTrans(n, q, p)
    others = {name: nttmul.NttCtMul(n, q, p, lib_path=path) for name, path in args.libs}
    plain = [nttmul.Context(n, m) for m in q]
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)
    reps = args.reps or (5 if batch * dnum * M * n >= 1 << 26 else 50)

    key_hat = random_words(torch, gen, ext, (2, dnum), n, dtype)
    d2_hat = torch.empty((batch, L, n), dtype=dtype, device="cuda")
    up_hat = torch.empty((batch, dnum, M, n), dtype=dtype, device="cuda")
    c_hat = torch.empty((batch, 2, M, n), dtype=dtype, device="cuda")
    c_lt = torch.empty_like(c_hat)
    out = torch.empty((batch, 2, L, n), dtype=dtype, device="cuda")
    row = {"word_bits": bits, "n": n, "batch": batch, "batch_asked": asked, "q_limbs": L,
           "p_limbs": K, "digit_limbs": alpha, "digits": dnum, "reps": reps, "pairs": []}
    hashes = nttmul.kernel_hashes(nttmul.CTMUL_LIB_PATH)
    names = [ct.kernel_name("high"), ct.kernel_name("relin"), lt.kernel_name(2, False)]
    row["kernel_hashes"] = {k: hashes[nttmul.dispatch_key(k)] for k in names}
    poly = batch * n * wb

    def chain_on(xs, ys, pairs):
        ct.high_device(d2_hat, xs, ys, batch, pairs, stream=stream)
        kn.modup_device(up_hat, d2_hat, batch, stream=stream)
        ct.relin_device(c_hat, up_hat, key_hat, xs, ys, batch, pairs, dnum, stream=stream)
        md.moddown_device(out, c_hat, batch * 2, stream=stream)

    for pairs in pair_counts:
        x_hat = random_words(torch, gen, q, (batch, pairs, 2), n, dtype)
        y_hat = random_words(torch, gen, q, (batch, pairs, 2), n, dtype)
        x_one, y_one = x_hat[:, :1].contiguous(), y_hat[:, :1].contiguous()
        high_polys = (2 * pairs + 1) * L
        relin_polys = (dnum + 2) * M + 4 * pairs * L
        copies = {k: (torch.empty(batch * v * n // 2, dtype=dtype, device="cuda"),
                      torch.empty(batch * v * n // 2, dtype=dtype, device="cuda"))
                  for k, v in (("high_copy", high_polys), ("relin_copy", relin_polys),
                               ("xy_copy", 4 * pairs * L))}

        def high_new():
            ct.high_device(d2_hat, x_hat, y_hat, batch, pairs, stream=stream)

        def relin_new():
            ct.relin_device(c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, dnum,
                            stream=stream)

        def apply_today():
            lt.apply_device(c_lt, up_hat, key_hat, (1,), batch, dnum, 2, stream=stream)

        def copier(name):
            dst, src = copies[name]
            return lambda: dst.copy_(src, non_blocking=True)

        high_new()
        kn.modup_device(up_hat, d2_hat, batch, stream=stream)
        relin_new()
        chk = min(batch, CHECK_ENTRIES)
        d2_want, c_want = composition(torch, kn, plain, up_hat[:chk], key_hat, x_hat[:chk],
                                      y_hat[:chk], q, p, bits)
        torch.cuda.synchronize()
        assert torch.equal(d2_hat[:chk], d2_want), "high differs from the composition"
        assert torch.equal(c_hat[:chk], c_want), "relin differs from the composition"
        del d2_want, c_want
        relins = {"relin": relin_new}
        for name, ctx in others.items():
            def relin_other(ctx=ctx):
                ctx.relin_device(c_lt, up_hat, key_hat, x_hat, y_hat, batch, pairs, dnum,
                                 stream=stream)
            relin_other()
            torch.cuda.synchronize()
            assert torch.equal(c_lt, c_hat), f"relin_{name} differs from relin"
            relins[f"relin_{name}"] = relin_other
        st = timed(torch, {"high": high_new, "high_copy": copier("high_copy")}, args.rounds, reps,
                   args.warmup)
        st.update(timed(torch, {**relins, "apply": apply_today,
                                "relin_copy": copier("relin_copy"), "xy_copy": copier("xy_copy")},
                        args.rounds, reps, args.warmup))
        st.update(timed(torch, {"chain": lambda: chain_on(x_hat, y_hat, pairs),
                                "chain_each": lambda: [chain_on(x_one, y_one, 1)
                                                       for _ in range(pairs)]},
                        args.rounds, max(1, reps // 2), args.warmup))
        allowed = st["apply"]["median"] + st["xy_copy"]["median"]
        row["pairs"].append({
            "pairs": pairs, "ms": st,
            "copy_tbps": {k: round(v * poly / (st[k]["median"] * 1e-3) / 1e12, 3)
                          for k, v in (("high_copy", high_polys), ("relin_copy", relin_polys),
                                       ("xy_copy", 4 * pairs * L))},
            "high": {"bytes": high_polys * poly,
                     "median_over_copy": round(st["high"]["median"] / st["high_copy"]["median"], 3),
                     **ratio_of(st, "high", "high_copy")},
            "relin": {"bytes": relin_polys * poly,
                      "median_over_bound": round(st["relin"]["median"] /
                                                 st["relin_copy"]["median"], 3),
                      "median_over_apply": round(st["relin"]["median"] / st["apply"]["median"], 3),
                      "apply_plus_xy_copy_ms": round(allowed, 5),
                      "costs_more_than_apply_plus_copy": bool(st["relin"]["median"] > allowed),
                      "other_over_relin": {k: round(st[k]["median"] / st["relin"]["median"], 3)
                                           for k in st if k.startswith("relin_") and
                                           k != "relin_copy"},
                      **ratio_of(st, "relin", "apply")},
            "chain": {**ratio_of(st, "chain", "chain_each"),
                      "launches": {"new": 6 if n <= 4096 else 10,
                                   "each": pairs * (6 if n <= 4096 else 10)}}})
        del x_hat, y_hat, x_one, y_one, copies
        torch.cuda.empty_cache()
    for h in (kn, md, ct, lt, *others.values(), *plain):
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


def parse_libs(text):
    libs = []
    for item in filter(None, text.split(",")):
        name, path = item.split("=")
        path = path if os.path.isabs(path) else os.path.join(
            ROOT, "ntt-based-polynomial-multiplier-fpga_amd", path)
        if not os.path.exists(path):
            raise ValueError(f"{path} not built: make ab-ctmul")
        if name == "copy":
            raise ValueError("a library named copy would shadow relin_copy")
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
    ap.add_argument("--pairs", default="1,4", help="comma-separated pair counts")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="sequences per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mem-gib", type=int, default=48,
                    help="the batch of a row is halved until its buffers fit this many GiB")
    ap.add_argument("--lib", default="",
                    help="comma-separated name=path of other builds of the library (relative to "
                         "the package directory), e.g. v2=lib/ab/libnttmul_ctmul_v2.so")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
        args.pair_list = [int(v) for v in args.pairs.split(",")]
        if not args.pair_list or min(args.pair_list) < 1:
            raise ValueError("pair counts are positive")
        args.libs = parse_libs(args.lib)
    except ValueError as e:
        ap.error(f"--rows / --pairs / --lib: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctmul.py measures on a GPU; none is visible")
    line = {"bench": "ctmul", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
            "warmup": args.warmup, "mem_gib": args.mem_gib,
            "libs": [name for name, _ in args.libs], "rows": []}
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
