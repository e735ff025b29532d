"""Generates tests/golden/capi_refusals_parent.json: what every chain-launch
and kernel-name entry of the C ABI answers to a call with something wrong --
(return code, hyg_last_error()) per case -- recorded from the library of the
commit before capi.cpp's host launch layer was folded into shared helpers (run
from the repo root against that library: ``HYG_LIB_PATH=/path/to/libhygeia_amd.so
python tests/golden/make_capi_refusals.py``).

Two sections, each recorded where it can be: ``no_device`` on a host without a
GPU, where everything behind an entry's device check reads "no CPU fallback"
(so the section pins which refusals come before that check), and ``device`` on
the MI355X, where the refusals behind the check become reachable (workspace one
byte short, null output buffers, psi_capacity, the estimation settings,
n_chains == 0 returning HYG_OK). A run rewrites the section of the host it runs
on and keeps the other.

Every case has one thing wrong (a few have two, whose order the code defines)
and returns before anything is enqueued: no case reaches a kernel launch. The
cases are only those the parent refuses: a chain argument that an entry does
not look at (a negative out_begin in an untraced forward-only launch), or one
that a host form refuses only after its emission kernel ran (a chain longer than
max_duration), is not a case. On a device the buffers are real allocations of
the sizes a valid call needs.

tests/test_capi_refusals_cpu.py and tests/test_gpu_capi_refusals.py replay
run() on the library under test and compare case by case.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "capi_refusals_parent.json")

# the smallest valid models; chains of 1-3 sites
K, MAX_READS, MAX_DURATION = 2, 4, 4
N_SITES = OUT_ROWS = 6
CHAINS = ((0, 3, 1, 0, 0), (3, 2, 2, 1, 3))  # site_begin, n_sites, seed, chain_id, out_begin

TG = {
    "hyg_tg_run_chains": "m chains n_chains E ws wsb out stream",
    "hyg_tg_run_chains_multi": "models n_models chains chain_model n_chains E ws wsb_multi out stream",
    "hyg_tg_filter_chains": "m chains n_chains E ws fwsb log_z final_w status stream",
    "hyg_tg_filter_chains_multi":
        "models n_models chains chain_model n_chains E ws fwsb_multi log_z final_w status stream",
    "hyg_tg_trace_chains": "m chains n_chains E ws fwsb trace log_z final_w status stream",
    "hyg_tg_trace_chains_multi":
        "models n_models chains chain_model n_chains E ws fwsb_multi trace log_z final_w status stream",
    "hyg_tg_run_chains_host":
        "m meth_c tot_c s_c meth_k tot_k s_k n_sites chains n_chains out_rows h_merged h_control h_kase h_split "
        "h_regime h_log_z h_final_w h_status",
    "hyg_tg_run_chains_host_multi":
        "models n_models meth_c tot_c s_c meth_k tot_k s_k n_sites chains chain_model n_chains out_rows h_merged "
        "h_control h_kase h_split h_regime h_log_z h_final_w h_status",
    "hyg_tg_filter_chains_host":
        "m meth_c tot_c s_c meth_k tot_k s_k n_sites chains n_chains h_log_z h_final_w h_status",
    "hyg_tg_filter_chains_host_multi":
        "models n_models meth_c tot_c s_c meth_k tot_k s_k n_sites chains chain_model n_chains h_log_z h_final_w "
        "h_status",
    "hyg_tg_trace_chains_host":
        "m meth_c tot_c s_c meth_k tot_k s_k n_sites chains n_chains out_rows h_log_z_t h_split h_regime h_log_z "
        "h_final_w h_status",
    "hyg_tg_trace_chains_host_multi":
        "models n_models meth_c tot_c s_c meth_k tot_k s_k n_sites chains chain_model n_chains out_rows h_log_z_t "
        "h_split h_regime h_log_z h_final_w h_status",
    "hyg_tg_run_chain_host":
        "m meth_c tot_c s_c meth_k tot_k s_k T seed chain_id h_merged h_control h_kase h_split h_regime h_log_z "
        "h_final_w",
    "hyg_tg_kernel_name": "m n_chains backward buf len",
    "hyg_tg_kernel_name_multi": "models n_models n_chains backward buf len",
    "hyg_tg_filter_kernel_name": "m n_chains buf len",
    "hyg_tg_filter_kernel_name_multi": "models n_models n_chains buf len",
    "hyg_tg_trace_kernel_name": "m n_chains buf len",
    "hyg_tg_trace_kernel_name_multi": "models n_models n_chains buf len",
    "hyg_tg_models_compatible": "models n_models",
}

SG = {
    "hyg_sg_run_chains": "m chains n_chains E ws wsb psi regime_probs status stream",
    "hyg_sg_run_chains_pe": "m pe chains n_chains E ws wsb_pe psi regime_probs theta_out status stream",
    "hyg_sg_run_chains_multi":
        "models n_models chains chain_model n_chains E ws wsb_multi psi regime_probs status stream",
    "hyg_sg_run_chains_pe_multi":
        "models n_models pe chains chain_model n_chains E ws wsb_pe_multi psi regime_probs theta_out status stream",
    "hyg_sg_run_chain_host": "m meth tot S T seed chain_id h_regime_probs",
    "hyg_sg_run_chain_host_pe": "m pe meth tot S T seed chain_id h_regime_probs h_theta_out",
    "hyg_sg_run_chains_host_multi":
        "models n_models pe meth tot S n_sites chains chain_model n_chains out_rows h_regime_probs h_theta_out "
        "h_status",
    "hyg_sg_filter_chains": "m chains n_chains E ws fwsb log_z final_lw final_st n_part status stream",
    "hyg_sg_filter_chains_multi":
        "models n_models chains chain_model n_chains E ws fwsb_multi log_z final_lw final_st n_part status stream",
    "hyg_sg_trace_chains": "m chains n_chains E ws fwsb trace log_z final_lw final_st n_part status stream",
    "hyg_sg_trace_chains_multi":
        "models n_models chains chain_model n_chains E ws fwsb_multi trace log_z final_lw final_st n_part status "
        "stream",
    "hyg_sg_filter_chains_host_multi":
        "models n_models meth tot S n_sites chains chain_model n_chains h_log_z h_final_lw h_final_st h_n_part "
        "h_status",
    "hyg_sg_trace_chains_host_multi":
        "models n_models meth tot S n_sites chains chain_model n_chains out_rows h_log_z_t h_regime_probs h_cp_probs "
        "h_log_z h_final_lw h_final_st h_n_part h_status",
    "hyg_sg_filter_kernel_name": "m buf len",
    "hyg_sg_filter_kernel_name_multi": "models n_models buf len",
    "hyg_sg_trace_kernel_name": "m buf len",
    "hyg_sg_trace_kernel_name_multi": "models n_models buf len",
    "hyg_sg_models_compatible": "models n_models",
}

# The pointers an entry refuses when null (an optional one -- final_w, a device
# form's status, the stream -- is no case: the launch would run).
REQUIRED = ("m models chains chain_model E ws out log_z trace pe regime_probs theta_out meth_c tot_c meth_k tot_k "
            "meth tot h_merged h_control h_kase h_split h_regime h_log_z h_status h_regime_probs h_theta_out").split()
SIZES = "n_sites n_chains out_rows s_c s_k S T n_models".split()
OUT_MEMBERS = ("merged", "control", "kase", "split_probs", "regime_probs", "log_z")


class Ctx:
    """The library, the models and the buffers of one run (kept alive here)."""

    def __init__(self, lib, device: bool):
        self.lib, self.device, self.keep, self.models = lib, device, [], []

    def dbuf(self, n: int = 1 << 16) -> int:
        """A device buffer where there is a device, else an address no call reads."""
        if self.device:
            import torch

            t = torch.zeros(max(int(n), 1), dtype=torch.uint8, device="cuda")
            self.keep.append(t)
            return t.data_ptr()
        b = C.create_string_buffer(16)
        self.keep.append(b)
        return C.addressof(b)

    def hbuf(self, n: int = 1 << 16) -> int:
        a = np.zeros(n, np.uint8)
        self.keep.append(a)
        return a.ctypes.data

    def counts(self, value: int) -> np.ndarray:
        a = np.full((N_SITES, 1), value, np.uint16)
        self.keep.append(a)
        return a

    def tg_model(self, **kw):
        from hygeia_amd import _lib

        k = kw.pop("K", K)
        reads = kw.pop("max_total_reads", MAX_READS)
        mu, sigma = kw.pop("mu", [0.9, 0.1, 0.5][:k]), kw.pop("sigma", [0.05, 0.05, 0.1][:k])
        theta = [0.0] * (k * (k - 1)) + [math.log(4.0)] * k
        args = dict(minimum_duration=1, num_resampled_ancestors=2, num_samples_backward=1)
        args.update(kw)
        p = _lib.make_params(mu, sigma, theta, **args)
        h = C.c_void_p()
        rc = self.lib.hyg_tg_model_create(C.byref(p), reads, MAX_DURATION, C.byref(h))
        assert rc == 0, self.lib.hyg_last_error()
        self.models.append((self.lib.hyg_tg_model_destroy, h))
        return h.value

    def sg_model(self, **kw):
        from hygeia_amd import _lib

        k = kw.pop("K", K)
        reads = kw.pop("max_total_reads", MAX_READS)
        p = _lib.SgParams()
        self.lib.hyg_sg_params_default(C.byref(p))
        p.n_regimes, p.minimum_duration, p.num_particles_max = k, 1, 3 if k == K else k + 1
        fixed = kw.pop("is_kappa_fixed", 1)
        p.is_kappa_fixed, p.theta_len = fixed, k * k + (0 if fixed else k)
        for i in range(k * (k - 1)):
            p.theta[i] = 0.0
        for i in range(k * (k - 1), p.theta_len):
            p.theta[i] = math.log(4.0) if i < k * k else 0.5
        for name, v in kw.items():
            if name in ("alpha", "beta"):
                getattr(p, name)[0] = v
            else:
                setattr(p, name, v)
        h = C.c_void_p()
        rc = self.lib.hyg_sg_model_create(C.byref(p), reads, MAX_DURATION, C.byref(h))
        assert rc == 0, self.lib.hyg_last_error()
        self.models.append((self.lib.hyg_sg_model_destroy, h))
        return h.value

    def close(self):
        for destroy, h in self.models:
            destroy(h)
        self.models, self.keep = [], []


def handles(*hs):
    return (C.c_void_p * len(hs))(*hs)


def chain_array(cls, chains=CHAINS, **change):
    """The chain array; change: field -> value of chain 1."""
    arr = (cls * len(chains))()
    for i, (site_begin, n_sites, seed, chain_id, out_begin) in enumerate(chains):
        arr[i].site_begin, arr[i].n_sites, arr[i].seed, arr[i].chain_id, arr[i].out_begin = (
            site_begin, n_sites, seed, chain_id, out_begin)
    for field, v in change.items():
        setattr(arr[1], field, v)
    return arr


def index(*ks):
    return (C.c_int32 * len(ks))(*ks)


def common_pool(ctx: Ctx, chain_cls):
    p = {k: ctx.hbuf() for k in REQUIRED + ["h_final_w", "h_log_z_t", "h_final_lw", "h_final_st", "h_n_part",
                                            "h_cp_probs"] if k.startswith("h_")}
    p.update(chains=chain_array(chain_cls), chain_model=index(0, 1), n_chains=len(CHAINS), n_models=2,
             n_sites=N_SITES, out_rows=OUT_ROWS, stream=None, E=ctx.dbuf(), log_z=ctx.dbuf(), status=ctx.dbuf(),
             T=3, seed=1, chain_id=0, buf=C.create_string_buffer(256), len=256, backward=0)
    return p


def tg_pool(ctx: Ctx):
    from hygeia_amd import _lib

    L = ctx.lib
    p = common_pool(ctx, _lib.TgChain)
    m, m1 = ctx.tg_model(), ctx.tg_model(omega_case=0.7)
    models = handles(m, m1)
    steps = sum(c[1] for c in CHAINS)
    out = _lib.TgOutputs(*[ctx.dbuf() for _ in range(8)])
    p.update(m=m, models=models, out=out, final_w=ctx.dbuf(), s_c=1, s_k=1,
             meth_c=ctx.counts(0).ctypes.data, tot_c=ctx.counts(1).ctypes.data,
             meth_k=ctx.counts(0).ctypes.data, tot_k=ctx.counts(1).ctypes.data,
             trace=_lib.TgTrace(ctx.dbuf(), ctx.dbuf(), ctx.dbuf()),
             wsb=L.hyg_tg_workspace_bytes(m, 2, steps), wsb_multi=L.hyg_tg_workspace_bytes_multi(models, 2, 2, steps),
             fwsb=L.hyg_tg_filter_workspace_bytes(m, 2), fwsb_multi=L.hyg_tg_filter_workspace_bytes_multi(models, 2, 2))
    p["ws"] = ctx.dbuf(max(p["wsb"], p["wsb_multi"]) + 4096)
    return p


def sg_pool(ctx: Ctx):
    from hygeia_amd import _lib

    L = ctx.lib
    p = common_pool(ctx, _lib.SgChain)
    m, m1 = ctx.sg_model(), ctx.sg_model(epsilon=0.02)
    models = handles(m, m1)
    pe = _lib.SgPeParams()
    L.hyg_sg_pe_params_default(C.byref(pe))
    pe.n_steps_without_update = 2
    ch = p["chains"]
    p.update(m=m, models=models, pe=pe, psi=0, S=1, meth=ctx.counts(0).ctypes.data, tot=ctx.counts(1).ctypes.data,
             regime_probs=ctx.dbuf(), theta_out=ctx.dbuf(), final_lw=ctx.dbuf(), final_st=ctx.dbuf(),
             n_part=ctx.dbuf(), trace=_lib.SgTrace(ctx.dbuf(), ctx.dbuf(), ctx.dbuf()),
             wsb=L.hyg_sg_workspace_bytes(m, 2, 0), wsb_pe=L.hyg_sg_pe_workspace_bytes(m, ch, 2, 0),
             wsb_multi=L.hyg_sg_workspace_bytes_multi(models, 2, 2, 0),
             wsb_pe_multi=L.hyg_sg_pe_workspace_bytes_multi(models, 2, ch, 2, 0),
             fwsb=L.hyg_sg_filter_workspace_bytes(m, 2), fwsb_multi=L.hyg_sg_filter_workspace_bytes_multi(models, 2, 2))
    p["ws"] = ctx.dbuf(max(p["wsb_pe"], p["wsb_pe_multi"]) + 4096)
    return p


def is_launch(entry: str) -> bool:
    return "_chain" in entry


def is_host(entry: str) -> bool:
    return "_host" in entry


def traced(entry: str) -> bool:
    return "_trace_" in entry


def smoothing(entry: str) -> bool:
    return "_run_chain" in entry


def cases_of(entry: str, sig, pool, ctx: Ctx, family: str):
    """Yields (label, overrides) for one entry."""
    from hygeia_amd import _lib

    chain_cls = _lib.TgChain if family == "tg" else _lib.SgChain
    optional = ["pe"] if entry == "hyg_sg_run_chains_host_multi" else []  # (no pe: no estimation)
    if "h_log_z_t" in sig:
        optional += ["h_split", "h_regime", "h_regime_probs"]  # one trace array is enough
    for k in sig:
        if k in REQUIRED and k not in optional:
            yield "null_" + k, {k: None}
        if k in SIZES and (is_launch(entry) or k == "n_models"):
            for v in (0, -1):
                if k in ("s_c", "s_k", "S") and v == 0:
                    continue  # no samples in a group is a valid call
                yield f"{k}_{v}", {k: v}
    if "len" in sig:
        yield "len_-1", {"len": -1}
        yield "len_-1_null_model", {"len": -1, ("m" if "m" in sig else "models"): None}
    if "models" in sig:
        make = ctx.tg_model if family == "tg" else ctx.sg_model
        yield "null_model_0", {"models": handles(None, pool["models"][1])}
        yield "null_model_1", {"models": handles(pool["models"][0], None)}
        fields = (dict(K=3), dict(minimum_duration=2), dict(num_resampled_ancestors=3), dict(num_samples_backward=2),
                  dict(optimal_resampling=False), dict(max_total_reads=5), dict(mu=[0.9, 0.2]),
                  dict(sigma=[0.05, 0.06])) if family == "tg" else (
                      dict(K=3), dict(minimum_duration=2), dict(num_particles_max=4), dict(is_kappa_fixed=0),
                      dict(max_total_reads=5), dict(alpha=2.5), dict(beta=2.5))
        every = entry.endswith("models_compatible") or entry.endswith("_run_chains_multi")
        for kw in fields if every else fields[:1]:
            yield "models_differ_in_" + next(iter(kw)), {"models": handles(pool["models"][0], make(**dict(kw)))}
    if "chain_model" in sig:
        yield "chain_model_-1", {"chain_model": index(0, -1)}
        yield "chain_model_2", {"chain_model": index(2, 0)}
    if not is_launch(entry):
        return
    if "chains" in sig:
        yield "chain_no_sites", {"chains": chain_array(chain_cls, n_sites=0)}
        yield "chain_neg_site_begin", {"chains": chain_array(chain_cls, site_begin=-1)}
        if smoothing(entry) or traced(entry):
            yield "chain_neg_out_begin", {"chains": chain_array(chain_cls, out_begin=-1)}
        if not is_host(entry) or (family == "sg" and not smoothing(entry)):
            yield "chain_too_long", {
                "chains": chain_array(chain_cls, site_begin=0, out_begin=0, n_sites=MAX_DURATION + 1)}
        if is_host(entry):
            yield "chain_outside_sites", {"chains": chain_array(chain_cls, site_begin=4, n_sites=3, out_begin=0)}
            if "out_rows" in sig:
                yield "chain_outside_rows", {"chains": chain_array(chain_cls, site_begin=0, out_begin=4, n_sites=3)}
    for k in sig:
        if k.startswith("wsb") or k.startswith("fwsb"):
            # the launch's own size less one byte (less the 256 of slack that hyg_tg_workspace_bytes adds)
            short = pool[k] - (257 if family == "tg" and k.startswith("wsb") else 1)
            yield "workspace_one_byte_short", {k: short}
            yield "workspace_0", {k: 0}
            yield "workspace_short_and_null_E", {k: short, "E": None}
            yield "workspace_short_and_chain_too_long", {
                k: short, "chains": chain_array(chain_cls, site_begin=0, n_sites=MAX_DURATION + 1)}
            if "trace" in sig:
                yield "empty_trace_and_workspace_short", {k: short, "trace": type(pool["trace"])()}
            if "psi" in sig:
                yield "psi_capacity_-1_and_workspace_short", {k: short, "psi": -1}
    if "trace" in sig:
        yield "empty_trace", {"trace": type(pool["trace"])()}
        yield "empty_trace_and_null_chains", {"trace": type(pool["trace"])(), "chains": None}
        if "chain_model" in sig:
            yield "empty_trace_and_chain_model_2", {"trace": type(pool["trace"])(), "chain_model": index(2, 0)}
    if "h_log_z_t" in sig:
        none = {k: None for k in ("h_log_z_t", "h_split", "h_regime", "h_regime_probs", "h_cp_probs") if k in sig}
        yield "empty_trace", none
        yield "empty_trace_and_out_rows_0", dict(none, out_rows=0)
    if "out" in sig:
        for member in OUT_MEMBERS:
            o = _lib.TgOutputs(*[getattr(pool["out"], f) for f, _ in _lib.TgOutputs._fields_])
            setattr(o, member, None)
            yield "null_out_" + member, {"out": o}
        if "m" in sig:
            yield "optimal_resampling_0", {"m": ctx.tg_model(optimal_resampling=False)}
    if family == "tg" and "m" in sig and not is_host(entry) and not smoothing(entry):
        yield "optimal_resampling_0", {"m": ctx.tg_model(optimal_resampling=False)}
    if "meth_c" in sig:
        yield "control_meth_above_tot", {"meth_c": ctx.counts(2).ctypes.data}
        yield "control_tot_above_max", {"tot_c": ctx.counts(MAX_READS + 1).ctypes.data}
        yield "case_meth_above_tot", {"meth_k": ctx.counts(2).ctypes.data}
        yield "case_tot_above_max", {"tot_k": ctx.counts(MAX_READS + 1).ctypes.data}
        yield "s_c_-1_and_null_log_z", {"s_c": -1, "h_log_z": None}
        if "chains" in sig:
            yield "null_meth_c_and_chain_outside_sites", {
                "meth_c": None, "chains": chain_array(chain_cls, site_begin=4, n_sites=3, out_begin=0)}
            yield "case_tot_above_max_and_chain_outside_sites", {
                "tot_k": ctx.counts(MAX_READS + 1).ctypes.data,
                "chains": chain_array(chain_cls, site_begin=4, n_sites=3, out_begin=0)}
    if "tot" in sig:
        yield "tot_above_max", {"tot": ctx.counts(MAX_READS + 1).ctypes.data}
    if "psi" in sig:
        yield "psi_capacity_-1", {"psi": -1}
        yield "psi_capacity_above_2^24", {"psi": (1 << 24) + 1}
    if "pe" in sig:
        pe = _lib.SgPeParams()
        ctx.lib.hyg_sg_pe_params_default(C.byref(pe))
        pe.n_steps_without_update = 0
        yield "n_steps_without_update_0", {"pe": pe}
        if "S" in sig:
            yield "n_steps_without_update_0_and_tot_above_max", {
                "pe": pe, "tot": ctx.counts(MAX_READS + 1).ctypes.data}
        if not is_host(entry):
            nan = _lib.SgPeParams()
            ctx.lib.hyg_sg_pe_params_default(C.byref(nan))
            nan.learning_rate_factor = float("nan")
            yield "learning_rate_nan", {"pe": nan}
            for k in sig:
                if k.startswith("wsb"):
                    yield "learning_rate_nan_and_workspace_short", {"pe": nan, k: pool[k] - 1}
    if family == "sg" and "log_z" in sig:
        yield "null_log_z_and_chain_no_sites", {"log_z": None, "chains": chain_array(chain_cls, n_sites=0)}
    if entry.endswith("_multi") and "E" in sig and "chains" in sig:
        other = ctx.tg_model(K=3) if family == "tg" else ctx.sg_model(K=3)
        yield "models_differ_and_null_chains", {"models": handles(pool["models"][0], other), "chains": None}


def run(lib, device: bool):
    """{case name: [return code, message]} over every case, on `lib`. The
    message of a call that refuses nothing (a kernel name, n_chains == 0 on a
    device) is "": hyg_last_error() then still holds an earlier one."""
    got = {}
    for family, table, make_pool in (("tg", TG, tg_pool), ("sg", SG, sg_pool)):
        ctx = Ctx(lib, device)
        try:
            pool = make_pool(ctx)
            for entry, text in table.items():
                sig = text.split()
                fn = getattr(lib, entry)
                for label, change in cases_of(entry, sig, pool, ctx, family):
                    assert all(k in sig for k in change), (entry, label)
                    args = [change[k] if k in change else pool[k] for k in sig]
                    rc = int(fn(*args))
                    name = f"{entry}:{label}"
                    assert name not in got, name
                    got[name] = [rc, lib.hyg_last_error().decode() if rc < 0 else ""]
        finally:
            ctx.close()
    return got


def main() -> None:
    from hygeia_amd import _lib

    lib = _lib.load()
    device = lib.hyg_device_count() > 0
    doc = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    section = "device" if device else "no_device"
    doc[section] = run(lib, device)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    accepted = [k for k, v in doc[section].items() if v[0] >= 0]
    print(section, len(doc[section]), "cases;", len(accepted), "refuse nothing:")
    for k in accepted:
        print("  ", k, doc[section][k][0])


if __name__ == "__main__":
    main()
