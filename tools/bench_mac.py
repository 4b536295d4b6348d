"""Products against an NTT-domain operand, fused (lib/libnttmul_mac.so, nttmul_mac_ntt_device)
against the calls they replace (lib/libnttmul.so), device-resident, interleaved in one run:

    python tools/bench_mac.py [--n 4096] [--q 2013265921] [--batch 65536] [--rounds 9] [--reps 50]
                              [--warmup 3] [--out profiles/mac/bench.json]

Timed sequences (device events around `reps` back-to-back calls, one synchronise per window):
  mac_t1_shared / mac_t1_batch   one fused call, terms = 1, b_hat shared by the batch / per batch
  mac_t4_shared / mac_t4_batch   one fused call, terms = 4
  three_call_t1                  forward(a), pointwise(a_hat, b_hat), inverse: what a holder of
                                 b_hat calls today for one product (b_hat per batch: the pointwise
                                 call has no shared form)
  multiply_t1                    multiply_batch_device(a, b), which transforms b again
  multiply_x4                    four multiply_batch_device calls (terms = 4 without the additions,
                                 which the library cannot do on the device)
The variants run round-robin, `rounds` times, each round starting one variant later; the line
reports the median, minimum and maximum window of each (ms per call), the ratios of the medians,
and the kernel hashes of the kernels involved.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd"))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0],
                                 epilog="see the module docstring for the timed sequences")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--q", type=int, default=2013265921)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)

    import torch
    import nttmul
    if not torch.cuda.is_available():
        raise SystemExit("bench_mac.py measures on a GPU; none is visible")
    n, q, batch, T = args.n, args.q, args.batch, 4
    bits = 32 if q < (1 << 32) else 64
    dt = torch.int32 if bits == 32 else torch.int64
    mac = nttmul.MacContext(n, q)
    base = nttmul.Context(n, q)
    stream = torch.cuda.current_stream().cuda_stream

    def buf(polys):
        return torch.empty(polys * n, dtype=dt, device="cuda")

    a, b, b_hat = buf(batch * T), buf(batch * T), buf(batch * T)    # [batch][T][n]
    a1, b1, bh1 = buf(batch), buf(batch), buf(batch)                # [batch][1][n]
    c, a_hat, tmp = buf(batch), buf(batch), buf(batch)
    c4 = [buf(batch) for _ in range(T)]
    base.fill_random_device(a, b, 0, batch * T, bits, stream=stream)
    base.fill_random_device(a1, b1, batch * T, batch, bits, stream=stream)
    base.forward_device(b_hat, b, batch * T, bits, stream=stream)
    base.forward_device(bh1, b1, batch, bits, stream=stream)
    # a [batch][T][n] as T arrays [batch][n] for the plain products (a copy: the layouts differ)
    at = [x.contiguous() for x in a.view(batch, T, n).unbind(1)]
    bt = [x.contiguous() for x in b.view(batch, T, n).unbind(1)]

    def three_call():
        base.forward_device(a_hat, a1, batch, bits, stream=stream)
        base.pointwise_device(tmp, a_hat, bh1, batch, bits, stream=stream)
        base.inverse_device(c, tmp, batch, bits, stream=stream)

    def multiply_x4():
        for t in range(T):
            base.multiply_device(c4[t], at[t], bt[t], batch, bits, stream=stream)

    variants = {
        "mac_t1_shared": lambda: mac.mac_ntt_device(c, a1, bh1, batch, 1, bits, shared=True, stream=stream),
        "mac_t1_batch": lambda: mac.mac_ntt_device(c, a1, bh1, batch, 1, bits, stream=stream),
        "mac_t4_shared": lambda: mac.mac_ntt_device(c, a, b_hat, batch, T, bits, shared=True, stream=stream),
        "mac_t4_batch": lambda: mac.mac_ntt_device(c, a, b_hat, batch, T, bits, stream=stream),
        "three_call_t1": three_call,
        "multiply_t1": lambda: base.multiply_device(c, a1, b1, batch, bits, stream=stream),
        "multiply_x4": multiply_x4,
    }

    # the sequences compute the same thing (per-batch b_hat, terms = 1), bit for bit
    variants["mac_t1_batch"]()
    fused = c.clone()
    three_call()
    assert torch.equal(fused, c), "fused call and three-call sequence differ"
    variants["multiply_t1"]()
    assert torch.equal(fused, c), "fused call and plain product differ"
    variants["mac_t4_batch"]()
    fused4 = c.clone()
    multiply_x4()
    if q < (1 << 60):  # (the sum of four residues fits int64)
        def wide(x):
            return x.to(torch.int64) & 0xFFFFFFFF if bits == 32 else x
        acc = wide(c4[0]).clone()
        for t in range(1, T):
            acc += wide(c4[t])
        assert torch.equal(acc % q, wide(fused4)), "fused 4-term call and the sum of four products differ"
        del acc
    del fused, fused4

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
            for _ in range(args.reps):
                variants[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.reps)

    med = {k: statistics.median(v) for k, v in ms.items()}
    arith = "Arith32P" if q < (1 << 31) else "Arith32W" if q < (1 << 32) else "Arith64"
    io, logn = ("u32" if bits == 32 else "u64"), n.bit_length() - 1
    base_hashes = nttmul.kernel_hashes(nttmul.LIB_PATH)
    mac_hashes = nttmul.kernel_hashes(nttmul.MAC_LIB_PATH)
    base_keys = [f"k_xform<{arith},{io},{io},{logn},0,0>", f"k_xform<{arith},{io},{io},{logn},0,1>",
                 f"k_pointwise<{'Arith32' if arith == 'Arith32P' else arith},{io}>",
                 nttmul.dispatch_key(base.kernel_name(bits, batch))]
    mac_key = nttmul.dispatch_key(mac.mac_kernel_name(bits))
    line = {
        "bench": "mac_ntt", "device": torch.cuda.get_device_name(0), "n": n, "q": q, "batch": batch,
        "word_bits": bits, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
        "ms_per_call": {k: {"median": round(med[k], 4), "min": round(min(v), 4),
                            "max": round(max(v), 4)} for k, v in ms.items()},
        "ratios": {
            "three_call_t1/mac_t1_shared": round(med["three_call_t1"] / med["mac_t1_shared"], 3),
            "three_call_t1/mac_t1_batch": round(med["three_call_t1"] / med["mac_t1_batch"], 3),
            "multiply_t1/mac_t1_shared": round(med["multiply_t1"] / med["mac_t1_shared"], 3),
            "multiply_x4/mac_t4_shared": round(med["multiply_x4"] / med["mac_t4_shared"], 3),
            "multiply_x4/mac_t4_batch": round(med["multiply_x4"] / med["mac_t4_batch"], 3),
        },
        "kernel_hashes": {"libnttmul_mac.so": {mac_key: mac_hashes[mac_key]},
                          "libnttmul.so": {k: base_hashes[k] for k in base_keys}},
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
