"""The exact base extension and the rounded ModDown (lib/libnttmul_xconv.so) against the inexact
forms of the same commit and against device-to-device copies, interleaved in one run,
device-resident:

    python tools/bench_xconv.py [--rows 32:4096x16384:4x1,...] [--rounds 7] [--reps 0]
                                [--warmup 3] [--scale 1] [--out profiles/xconv/bench.json]

A row is bits:n x batch:L x K.  The default rows are tools/bench_mdntt.py's: n = 4096 x 16,384 and
n = 65536 x 1,024 in both word classes for (L, K) = (4, 1), (4, 2) and (12, 4), and the thin shape
n = 4096 x 64.  The bases are the first L primes = 1 mod 2^17 below the top of the class, then the
next K.  Per row two groups are timed (device events around `reps` back-to-back calls, one
synchronise per window), each group round-robin, `rounds` times, each round starting one variant
later:
  moddown   nttmul_xconv_moddown_device          the rounded form
  floor     nttmul_mdntt_moddown_device          the floor form: the same transforms, no correction
  copy_x    hipMemcpyAsync device to device of x_hat's bytes
  extend    nttmul_xconv_extend_device           K limbs -> L limbs, exact
  modup     nttmul_ksntt_modup_device with one digit of all K limbs as its Q and the L limbs as
            its P: the inexact raise with the same transforms (it also copies the K own limbs)
  copy_out  hipMemcpyAsync of extend's output's bytes
The line reports the median, minimum and maximum window of each (ms per call), the ratios
moddown / floor and extend / modup -- the price of exactness -- and the baselines' own spread
((max - min) / median), which a difference has to exceed to mean anything.  No threshold is set.
Before timing both operations are compared with the device composition of tests/xconv_gpu.py on
the first 33 batch entries.  --reps 0 picks 20 for rows of at least 2^26 coefficients and 200
below.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = ",".join(f"{bits}:{shape}:{lk}" for shape in ("4096x16384", "65536x1024")
                        for bits in (32, 64) for lk in ("4x1", "4x2", "12x4")) + \
    ",32:4096x64:4x1,64:4096x64:4x1"
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 65536
CHECKED = 33


def primes_below(nttmul, top, count):
    q, out = (top - 2) // STEP * STEP + 1, []
    while len(out) < count:
        if nttmul.is_prime(q):
            out.append(q)
        q -= STEP
    return out


def timed(torch, variants, rounds, reps, warmup):
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


def bench_row(torch, nttmul, bits, n, batch, L, K, args):
    from xconv_gpu import check_composition
    primes = primes_below(nttmul, TOP[bits], L + K)
    q, p = primes[:L], primes[L:]
    xc = nttmul.NttExactConv(n, q, p, args.scale)
    md = nttmul.NttModDown(n, q, p)
    up = nttmul.NttKeySwitch(n, p, q, K)          # one digit: the K limbs raised into the L
    stream = torch.cuda.current_stream().cuda_stream
    dtype = torch.int32 if bits == 32 else torch.int64
    np_view = (lambda t: t.cpu().numpy().view("uint32" if bits == 32 else "uint64"))
    gen = torch.Generator(device="cuda").manual_seed(L * 100 + K)
    x = torch.empty((batch, L + K, n), dtype=dtype, device="cuda")
    for l, m in enumerate(q + p):
        x[:, l, :] = torch.randint(0, m, (batch, n), generator=gen, device="cuda",
                                   dtype=torch.int64).to(dtype)
    ph = x[:, L:, :].contiguous()
    out, out2 = (torch.empty((batch, L, n), dtype=dtype, device="cuda") for _ in range(2))
    raised = torch.empty((batch, 1, K + L, n), dtype=dtype, device="cuda")
    xcopy, ocopy = torch.empty_like(x), torch.empty_like(out)

    down = {"moddown": lambda: xc.moddown_device(out, x, batch, stream=stream),
            "floor": lambda: md.moddown_device(out2, x, batch, stream=stream),
            "copy_x": lambda: xcopy.copy_(x, non_blocking=True)}
    raise_ = {"extend": lambda: xc.extend_device(out, ph, batch, stream=stream),
              "modup": lambda: up.modup_device(raised, ph, batch, stream=stream),
              "copy_out": lambda: ocopy.copy_(out2, non_blocking=True)}
    head = min(CHECKED, batch)
    down["moddown"]()
    torch.cuda.synchronize()
    check_composition("moddown", n, q, p, args.scale, np_view(x[:head]), np_view(out[:head]))
    raise_["extend"]()
    torch.cuda.synchronize()
    check_composition("extend", n, q, p, args.scale, np_view(ph[:head]), np_view(out[:head]))

    reps = args.reps or (20 if batch * n >= 1 << 26 else 200)
    stat = timed(torch, down, args.rounds, reps, args.warmup)
    stat.update(timed(torch, raise_, args.rounds, reps, args.warmup))
    spread = lambda k: round((stat[k]["max"] - stat[k]["min"]) / stat[k]["median"], 3)
    ratio = lambda a, b: round(stat[a]["median"] / stat[b]["median"], 3)
    hashes = nttmul.kernel_hashes(nttmul.XCONV_LIB_PATH)
    names = {op: xc.kernel_name(op).split(" + ") for op in ("extend", "moddown")}
    row = {"word_bits": bits, "n": n, "batch": batch, "q_limbs": L, "p_limbs": K, "reps": reps,
           "ms_per_call": stat,
           "moddown_over_floor": ratio("moddown", "floor"), "floor_spread": spread("floor"),
           "moddown_over_copy_x": ratio("moddown", "copy_x"),
           "extend_over_modup": ratio("extend", "modup"), "modup_spread": spread("modup"),
           "extend_over_copy_out": ratio("extend", "copy_out"),
           "kernels": {op: " + ".join(v) for op, v in names.items()},
           "kernel_hashes": {k: hashes[nttmul.dispatch_key(k)] for v in names.values() for k in v}}
    for h in (xc, md, up):
        h.close()
    return row


def parse_rows(text):
    rows = []
    for item in text.split(","):
        bits, shape, limbs = item.split(":")
        n, batch = (int(v) for v in shape.split("x"))
        L, K = (int(v) for v in limbs.split("x"))
        if int(bits) not in TOP:
            raise ValueError(f"word bits {bits}: 32 or 64")
        rows.append((int(bits), n, batch, L, K))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--rows", default=DEFAULT_ROWS,
                    help="comma-separated bits:n x batch:L x K, e.g. 32:4096x16384:4x1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=0, help="calls per window (0: by shape)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="the context's t")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    try:
        rows = parse_rows(args.rows)
    except ValueError as e:
        ap.error(f"--rows: {e}")

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_xconv.py measures on a GPU; none is visible")
    line = {"bench": "xconv", "device": torch.cuda.get_device_name(0),
            "library": os.path.relpath(nttmul.XCONV_LIB_PATH, ROOT), "rounds": args.rounds,
            "warmup": args.warmup, "scale": args.scale, "rows": []}
    for row in rows:
        line["rows"].append(bench_row(torch, nttmul, *row, args))
        print("row %s done" % (row,), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
