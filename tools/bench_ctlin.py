"""Ciphertext sums, plaintext products and the full tensor product (lib/libnttmul_ctlin.so) against
a device-to-device copy moving the same bytes and against the composition a caller runs today,
interleaved in one run per row, device-resident:

    python tools/bench_ctlin.py [--rows 32:4096x16384:6,...] [--rounds 7] [--reps 0] [--warmup 2]
                                [--mem-gib 48] [--out profiles/ctlin/bench.json]

A row is bits:n x batch:limbs, tools/bench_ctmul.py's shapes with Q u P as one basis: n = 4096 x
16,384 and n = 65536 x 1,024 in both word classes at 6 and 16 limbs, and the thin shape n = 4096 x
64.  The batch of a row is halved until the row's buffers fit --mem-gib; the row records the batch
it ran.  Per row the timed calls are (device events around `reps` back-to-back calls, one
synchronise per window), combine at comps = 2:
  add      ct + ct' (2 ONE terms)
  fma      pt o ct + ct' (PLAIN, ONE)
  dot4     sum of 4 pt_i o ct_i
  dot16    sum of 16 pt_i o ct_i
  tensor1  nttmul_ctlin_tensor_device at pairs = 1
  tensor4  at pairs = 4
each in a group with
  <call>_copy   a device-to-device copy moving the call's bytes ((terms + 1) comps L n w per entry
                for combine, (4 pairs + 3) L n w for tensor; plaintexts are shared by the batch and
                left out)
  <call>_today  the composition a caller runs without the library: per limb a contiguous slice
                and nttmul_pointwise_batch_device for every product, torch additions mod q_l
  <call>_int64  on 32-bit words only: the torch form, (x.long() * w.long()) % q_l and sums
The variants of a group run round-robin, `rounds` times, each round starting one variant later; the
line reports the median, minimum and maximum window of each (ms per call), the call over the copy,
the copy's own spread ((max - min) / median) and whether the call is behind the copy by more than
that spread, and the compositions over the call.  A copy of B bytes moves 2 B.  Before timing, each
call's result on the first entries of the batch (a partial last workgroup among them at small n)
is compared bit for bit with the composition.  --reps 0 picks 5 for rows of at least 2^26 words
per ciphertext and 50 below; the compositions run a fifth as often.  Prints one JSON line (and
writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ",".join(f"{bits}:{shape}:{limbs}" for shape in ("4096x16384", "65536x1024")
                        for bits in (32, 64) for limbs in (6, 16)) + ",32:4096x64:6,64:4096x64:6"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 65536
COMPS = 2
DOTS = (4, 16)
PAIRS = (1, 4)
CHECK_ENTRIES = 33          # verified against the composition: whole workgroups and one entry


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def row_polys(L):
    """Limb polynomials per batch entry of a row's buffers: 16 ciphertexts, the output, tensor's
    operands and output, the largest copy's source and target (half the largest call's bytes
    each), and as much again for the compositions' intermediates."""
    most = max((max(DOTS) + 1) * COMPS, 4 * max(PAIRS) + 3)
    return (max(DOTS) * COMPS + COMPS + 4 * max(PAIRS) + 3 + 2 * most) * L


def fit_batch(batch, L, n, wb, limit):
    while batch > 1 and batch * row_polys(L) * n * wb > limit:
        batch //= 2
    return batch


def random_words(torch, gen, moduli, lead, n, dtype):
    x = torch.empty((*lead, len(moduli), n), dtype=dtype, device="cuda")
    for l, m in enumerate(moduli):
        x[..., l, :] = torch.randint(0, m, (*lead, n), generator=gen, device="cuda",
                                     dtype=torch.int64).to(dtype)
    return x


def timed(torch, variants, rounds, reps, warmup):
    """{name: {median, min, max}} in ms per call, the variants interleaved round-robin.
    variants: {name: (fn, reps divisor)}."""
    for fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    names = list(variants)
    ms = {k: [] for k in names}
    for r in range(rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            fn, div = variants[k]
            count = max(1, reps // div)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / count)
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                "max": round(max(v), 5)} for k, v in ms.items()}


def addmod(torch, x, y, m):
    s = x.to(torch.int64) + y.to(torch.int64)
    return torch.where(s >= m, s - m, s).to(x.dtype)


class Today:
    """The compositions a caller runs without the library, on device-resident operands."""

    def __init__(self, torch, plain, q, n, bits):
        self.torch, self.plain, self.q, self.n, self.bits = torch, plain, q, n, bits

    def product(self, l, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = self.torch.empty_like(a)
        self.plain[l].pointwise_device(out, a, b, a.numel() // self.n, self.bits)
        return out

    def product_int64(self, l, a, b):
        return ((a.to(self.torch.int64) * b.to(self.torch.int64)) % self.q[l]).to(a.dtype)

    def combine(self, out, xs, ws, product):
        """out[:, :, l] = sum_i ws[i][l] o xs[i][:, :, l] (ws[i] None: weight 1)."""
        for l, m in enumerate(self.q):
            acc = None
            for x, w in zip(xs, ws):
                t = x[:, :, l] if w is None else product(l, x[:, :, l], w[l].expand_as(x[:, :, l]))
                acc = t if acc is None else addmod(self.torch, acc, t, m)
            out[:, :, l] = acc

    def tensor(self, out, x, y, product):
        pairs = x.shape[1]
        for l, m in enumerate(self.q):
            x0, x1, y0, y1 = x[:, :, 0, l], x[:, :, 1, l], y[:, :, 0, l], y[:, :, 1, l]
            sums = []
            for a, b in ((x0, y0), (x0, y1), (x1, y0), (x1, y1)):
                pr = product(l, a, b)
                acc = pr[:, 0]
                for s in range(1, pairs):
                    acc = addmod(self.torch, acc, pr[:, s], m)
                sums.append(acc)
            out[:, 0, l], out[:, 2, l] = sums[0], sums[3]
            out[:, 1, l] = addmod(self.torch, sums[1], sums[2], m)


def bench_row(torch, nttmul, bits, n, batch, L, args):
    q = primes_below(nttmul, TOP[bits], L)
    wb = bits // 8
    asked = batch
    batch = fit_batch(batch, L, n, wb, args.mem_gib << 30)
    cl = nttmul.NttCtLin(n, q)
    plain = [nttmul.Context(n, m) for m in q]
    today = Today(torch, plain, q, n, bits)
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + n % 97)
    reps = args.reps or (5 if batch * COMPS * L * n >= 1 << 26 else 50)
    cts = [random_words(torch, gen, q, (batch, COMPS), n, dtype) for _ in range(max(DOTS))]
    pts = [random_words(torch, gen, q, (), n, dtype) for _ in range(max(DOTS))]
    out = torch.empty((batch, COMPS, L, n), dtype=dtype, device="cuda")
    d_hat = torch.empty((batch, 3, L, n), dtype=dtype, device="cuda")
    poly = batch * L * n * wb                   # bytes of one limb-polynomial set of the batch
    most = max((max(DOTS) + 1) * COMPS, 4 * max(PAIRS) + 3)
    pool = (torch.empty(most * poly // 2 // wb, dtype=dtype, device="cuda"),
            torch.empty(most * poly // 2 // wb, dtype=dtype, device="cuda"))
    row = {"word_bits": bits, "n": n, "batch": batch, "batch_asked": asked, "limbs": L,
           "comps": COMPS, "reps": reps, "calls": {}}
    hashes = nttmul.kernel_hashes(nttmul.CTLIN_LIB_PATH)
    names = [cl.kernel_name("combine", COMPS), cl.kernel_name("tensor")]
    row["kernel_hashes"] = {k: hashes[nttmul.dispatch_key(k)] for k in names}
    chk = min(batch, CHECK_ENTRIES)

    def copier(polys):
        words = polys * poly // 2 // wb
        dst, src = pool[0][:words], pool[1][:words]
        return lambda: dst.copy_(src, non_blocking=True)

    calls = {"add": ([cts[0], cts[1]], [None, None]), "fma": ([cts[0], cts[1]], [pts[0], None])}
    for k in DOTS:
        calls[f"dot{k}"] = (cts[:k], pts[:k])
    for name, (xs, ws) in calls.items():
        terms = [nttmul.ctlin_one(x) if w is None else nttmul.ctlin_plain(x, w)
                 for x, w in zip(xs, ws)]

        def new(terms=terms):
            cl.combine_device(out, terms, batch, COMPS, stream=stream)

        new()
        want = torch.empty_like(out[:chk])
        today.combine(want, [x[:chk] for x in xs], ws, today.product)
        torch.cuda.synchronize()
        assert torch.equal(out[:chk], want), f"{name} differs from the composition"
        polys = (len(xs) + 1) * COMPS
        group = {name: (new, 1), f"{name}_copy": (copier(polys), 1),
                 f"{name}_today": (lambda xs=xs, ws=ws: today.combine(out, xs, ws, today.product), 5)}
        if bits == 32:
            today.combine(want, [x[:chk] for x in xs], ws, today.product_int64)
            assert torch.equal(out[:chk], want), f"{name}: the int64 form differs"
            group[f"{name}_int64"] = (
                lambda xs=xs, ws=ws: today.combine(out, xs, ws, today.product_int64), 5)
        del want
        row["calls"][name] = summarise(timed(torch, group, args.rounds, reps, args.warmup), name,
                                       polys * poly)
    for pairs in PAIRS:
        name = f"tensor{pairs}"
        x = torch.stack([c for c in cts[:pairs]], dim=1)            # [batch, pairs, 2, L, n]
        y = torch.stack([c for c in cts[pairs:2 * pairs]], dim=1)

        def new(x=x, y=y, pairs=pairs):
            cl.tensor_device(d_hat, x, y, batch, pairs, stream=stream)

        new()
        want = torch.empty_like(d_hat[:chk])
        today.tensor(want, x[:chk], y[:chk], today.product)
        torch.cuda.synchronize()
        assert torch.equal(d_hat[:chk], want), f"{name} differs from the composition"
        polys = 4 * pairs + 3
        group = {name: (new, 1), f"{name}_copy": (copier(polys), 1),
                 f"{name}_today": (lambda x=x, y=y: today.tensor(d_hat, x, y, today.product), 5)}
        if bits == 32:
            today.tensor(want, x[:chk], y[:chk], today.product_int64)
            assert torch.equal(d_hat[:chk], want), f"{name}: the int64 form differs"
            group[f"{name}_int64"] = (
                lambda x=x, y=y: today.tensor(d_hat, x, y, today.product_int64), 5)
        del want
        row["calls"][name] = summarise(timed(torch, group, args.rounds, reps, args.warmup), name,
                                       polys * poly)
        del x, y
        torch.cuda.empty_cache()
    for h in (cl, *plain):
        h.close()
    return row


def summarise(st, name, nbytes):
    copy = st[f"{name}_copy"]
    spread = (copy["max"] - copy["min"]) / copy["median"]
    over = st[name]["median"] / copy["median"]
    out = {"ms": st, "bytes": nbytes,
           "copy_tbps": round(nbytes / (copy["median"] * 1e-3) / 1e12, 3),
           "median_over_copy": round(over, 3), "copy_spread": round(spread, 3),
           "behind_the_copy_by_more_than_its_spread": bool(over - 1 > spread),
           "today_over_call": round(st[f"{name}_today"]["median"] / st[name]["median"], 2)}
    if f"{name}_int64" in st:
        out["int64_over_call"] = round(st[f"{name}_int64"]["median"] / st[name]["median"], 2)
    return out


def parse_rows(text):
    rows = []
    for item in text.split(","):
        bits, shape, limbs = item.split(":")
        n, batch = (int(v) for v in shape.split("x"))
        if int(bits) not in TOP:
            raise ValueError(f"word bits {bits}: 32 or 64")
        rows.append((int(bits), n, batch, int(limbs)))
    return rows


def dump(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(obj) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed calls")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:limbs, e.g. 32:4096x16384:6")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mem-gib", type=int, default=48,
                    help="the batch of a row is halved until its buffers fit this many GiB")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
    except ValueError as e:
        ap.error(f"--rows: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctlin.py measures on a GPU; none is visible")
    line = {"bench": "ctlin", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
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
