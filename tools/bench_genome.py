"""A genome with per-chromosome models: one multi-model launch against the
alternatives.

Usage: python tools/bench_genome.py [--sites 28000000] [--repeats 3] [--out FILE.json]

The chains are bench.py's C3 workload (hg38-proportioned chromosomes, 100 k
segments + 5 k buffers, 2 seeds, 4 + 4 samples, K = 6, M = 50, B = 25) and
every chromosome has its own theta: uniform_theta perturbed per chromosome from
a fixed seed, as theta_{chrom}.csv.gz differs from chromosome to chromosome in
the pipeline. Three configurations run the same chains over the same counts,
the timed region as bench.py's launches (emission, forward, backward; a host
clock around work that ends in a stream synchronise):

  a  one multi-model launch (hyg_tg_run_chains_multi): every chain names its
     chromosome's model
  b  one single-model launch per chromosome, back to back on one stream: the
     only way before multi-model launches
  c  one single-model launch of all chains with one theta (bench.py's C3): the
     ceiling, which real per-chromosome theta cannot use
  d  a's multi-model launch with c's theta as every chromosome's model: the
     same chains doing the same work as c in the multi-model kernels

After one warm-up of each, the configurations alternate (a, b, c, d, a, ...)
for --repeats rounds; the line reports every time, the medians and the spread
(max - min) of each, and the kernels' own times (HIP events) of the
single-launch configurations. a passes when its times overlap c's (or lie
below them). a and c differ in two things, the kernels (one load of the model
at entry) and theta, which sets how many particles stay alive per step; d
against c holds theta fixed and shows the kernels' part alone. b / a is
reported. The log Z of every chain of a equals b's, and d's equals c's, bit
for bit (checked).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THETA_SEED = 20260101


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=28_000_000)
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--theta-sd", type=float, default=0.3, help="per-chromosome N(0, sd) added to uniform_theta")
    ap.add_argument("--configs", default="abcd", help="the configurations to run (b takes 16 x the others' time)")
    ap.add_argument("--out", default=None, help="also write the result there (profiles/genome_multi_model.json)")
    args = ap.parse_args()

    import torch

    from hygeia_amd import _lib, synthetic, two_group

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.load()
    K, M, B = 6, 50, 25
    data = synthetic.simulate_device(args.sites, args.samples, args.samples, K=K, coverage=100.0, device=dev)
    sizes = synthetic.chromosome_sizes(args.sites)
    segs = synthetic.segment_chains(sizes)
    n_chrom = len(sizes)
    # (chromosome, chain) longest first, as bench.py orders a launch
    allc = sorted(((ci, (s0, n, sd, (ci << 32) | b)) for sd in range(args.seeds)
                   for (ci, b, s0, n, r0, rl) in segs), key=lambda c: -c[1][1])
    units = args.seeds * sum(rl for (ci, b, s0, n, r0, rl) in segs)

    def with_rows(cs):
        out, rows = [], 0
        for (s0, n, sd, cid) in cs:
            out.append((s0, n, sd, cid, rows))
            rows += n
        return out, rows

    chains, n_out = with_rows([c for _, c in allc])
    chain_model = [ci for ci, _ in allc]
    max_reads = int(max(data["tot_control"].to(torch.int32).max().item() & 0xFFFF,
                        data["tot_case"].to(torch.int32).max().item() & 0xFFFF))
    mu, sg = synthetic.regime_params(K)
    rng = np.random.default_rng(THETA_SEED)
    uniform = two_group.uniform_theta(K, 0.8)
    thetas = [uniform + rng.normal(0.0, args.theta_sd, uniform.shape) for _ in range(n_chrom)]
    longest = max(c[1] for c in chains)
    kw = dict(num_resampled_ancestors=M, num_samples_backward=B)
    models = two_group.genome_models(thetas, mu, sg, max_reads, [longest] * n_chrom, **kw)
    ceiling = two_group.CaseControlModel(mu, sg, uniform, max_total_reads=max_reads, max_duration=longest, **kw)
    same = two_group.genome_models([uniform] * n_chrom, mu, sg, max_reads, [longest] * n_chrom, **kw)

    ws = torch.empty(two_group.DeviceChains.workspace_bytes(models, chains), dtype=torch.uint8, device=dev)
    dc_a = two_group.DeviceChains(models, chains, n_out, device=dev, workspace=ws, chain_model=chain_model)
    dc_c = two_group.DeviceChains(ceiling, chains, n_out, device=dev, workspace=ws)
    dc_d = two_group.DeviceChains(same, chains, n_out, device=dev, workspace=ws, chain_model=chain_model)
    dc_b, pos_b = [], []  # per chromosome: its launch, and its chains' positions in the whole launch
    for ci in range(n_chrom):
        pos = [i for i, m in enumerate(chain_model) if m == ci]
        cs, rows = with_rows([chains[i][:4] for i in pos])
        dc_b.append(two_group.DeviceChains(models[ci], cs, rows, device=dev, workspace=ws))
        pos_b.append(pos)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    E = torch.empty((args.sites, 2 * K), dtype=torch.float64, device=dev)
    cnt = (data["meth_control"], data["tot_control"], data["meth_case"], data["tot_case"])

    def run_a():
        dc_a.emission(*cnt, E=E, stream=sp)
        dc_a.run(E, stream=sp)

    def run_b():
        dc_b[0].emission(*cnt, E=E, stream=sp)  # (one table: the models share it)
        for d in dc_b:
            d.run(E, stream=sp)

    def run_c():
        dc_c.emission(*cnt, E=E, stream=sp)
        dc_c.run(E, stream=sp)

    def run_d():
        dc_d.emission(*cnt, E=E, stream=sp)
        dc_d.run(E, stream=sp)

    def timed(fn) -> float:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    L.hyg_set_kernel_timing(1)  # (as bench.py runs: events around the last launch's kernels)
    ms3 = (ctypes.c_float * 3)()
    configs = [(k, fn) for k, fn in (("a", run_a), ("b", run_b), ("c", run_c), ("d", run_d)) if k in args.configs]
    if not {"a", "c"} <= {k for k, _ in configs}:
        raise SystemExit("--configs must hold a and c")
    for _, fn in configs:  # warm-up: every kernel and width the timed rounds use
        timed(fn)
    ms = {k: [] for k in "abcd"}
    kms = {k: [] for k in "acd"}  # emission, forward, backward of the one launch
    for r in range(args.repeats):
        for k, fn in configs:
            ms[k].append(timed(fn))
            print(f"round {r} {k}: {ms[k][-1]:.1f} ms", file=sys.stderr, flush=True)
            if k in kms:
                _lib.check(L.hyg_tg_last_kernel_ms(ms3))
                kms[k].append([round(float(x), 2) for x in ms3])
    L.hyg_set_kernel_timing(0)
    ran = [dc_a, dc_c] + ([dc_d] if "d" in args.configs else []) + (dc_b if "b" in args.configs else [])
    for d in ran:
        if (d.status != 0).any().item():
            raise RuntimeError("chains failed")
    if "d" in args.configs and dc_d.log_z.cpu().numpy().tobytes() != dc_c.log_z.cpu().numpy().tobytes():
        raise RuntimeError("a chain's log Z differs between the multi-model and the single-model launch of one theta")
    lz_a = dc_a.log_z.cpu().numpy()
    for d, pos in zip(dc_b if "b" in args.configs else [], pos_b):
        if lz_a[pos].tobytes() != d.log_z.cpu().numpy().tobytes():
            raise RuntimeError("a chain's log Z differs between the multi-model launch and its chromosome's launch")

    def stats(v):
        if not v:
            return {"ms": []}  # not run (--configs)
        return {"ms": [round(x, 2) for x in v], "median_ms": round(float(np.median(v)), 2),
                "spread_ms": round(max(v) - min(v), 2),
                "site_seeds_per_s": round(units / (float(np.median(v)) / 1000.0))}

    def name(multi, n):
        buf = ctypes.create_string_buffer(96)
        out = []
        for backward in (0, 1):
            if multi:
                L.hyg_tg_kernel_name_multi(dc_a._handles, n_chrom, n, backward, buf, 96)
            else:
                L.hyg_tg_kernel_name(ceiling.handle, n, backward, buf, 96)
            out.append(buf.value.decode())
        return out

    a, b, c, d = ms["a"], ms["b"], ms["c"], ms["d"]
    line = {
        "tool": "tools/bench_genome.py", "device": torch.cuda.get_device_name(dev),
        "source_hash": __import__("hygeia_amd.build", fromlist=["source_hash"]).source_hash(),
        "workload": f"C3 chains: {args.sites} CpG over {n_chrom} chromosomes, 100k segments + 5k buffers, "
                    f"{args.samples}+{args.samples} samples, K={K}, M={M}, B={B}, {args.seeds} seeds, "
                    f"{len(chains)} chains; theta = uniform_theta + N(0, {args.theta_sd}) per chromosome "
                    f"(seed {THETA_SEED})",
        "timed_region": "emission + forward + backward, host clock to stream synchronise; 1 warm-up of each, "
                        f"then {args.repeats} alternating rounds a, b, c, d",
        "units_site_seeds": units,
        "a_one_multi_model_launch": dict(stats(a), kernels=name(True, len(chains)),
                                         emission_forward_backward_ms=kms["a"]),
        "b_one_launch_per_chromosome": dict(stats(b), launches=n_chrom,
                                            chains_per_launch=[len(p) for p in pos_b]),
        "c_one_theta_single_launch": dict(stats(c), kernels=name(False, len(chains)),
                                          emission_forward_backward_ms=kms["c"]),
        "d_multi_model_launch_with_c_theta": dict(stats(d), kernels=name(True, len(chains)),
                                                  emission_forward_backward_ms=kms["d"]),
        "a_over_c_median": round(float(np.median(a) / np.median(c)), 4),
        "d_over_c_median": round(float(np.median(d) / np.median(c)), 4) if d else None,
        "d_within_spread_of_c": bool(min(d) <= max(c)) if d else None,
        "b_over_a_median": round(float(np.median(b) / np.median(a)), 3) if b else None,
        "a_within_spread_of_c": bool(min(a) <= max(c)),
        "criterion": "a's times overlap c's or lie below them: min(a) <= max(c)",
        "log_z_a_equals_b": bool(b) or None, "log_z_d_equals_c": bool(d) or None,
    }
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)
            fh.write("\n")
    for m in models + same + [ceiling]:
        m.close()


if __name__ == "__main__":
    main()
