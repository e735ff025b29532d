"""Host-side mirror of the reference's two-group inference interface.

Reference (src/two_group): the model is built as
    CaseControlRegimeModel(n_methylation_regimes, mu, sigma, P_softmax_control,
        P_softmax_merged, omega_inv_logit_control, omega_inv_logit_case,
        minimum_duration, kappa_control, kappa_case, n_total_reads_control,
        n_total_reads_case)                      (hygeia/case_control_regime_model.py:47-74)
from the CLI flags and the single-group theta (run_inference_two_groups.py:110-167),
and inference is
    filter_and_smoother_algorithm.run(observations, ..., num_particles,
        num_resampled_ancestors, optimal_resampling=True, num_simulations)
      -> (BackwardSimulationResults(step, particle={'merged_state', 'control_state',
          'case_state'}), final_unnormalized_log_weights)      (filter_and_smoother_algorithm.py:38-138)

Here `CaseControlModel` holds the same parameters (as a C-ABI model handle with
its tables on the GPU) and `run()` has the same meaning and return structure.
Every computation runs in the HIP kernels of libhygeia_amd.so; there is no CPU
fallback (without a HIP device the library raises HygError(HYG_EDEVICE)).
"""
from __future__ import annotations

import collections
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

BackwardSimulationResults = collections.namedtuple("BackwardSimulationResults", ["step", "particle"])


def theta_to_matrix(theta: Sequence[float], K: int) -> Tuple[np.ndarray, np.ndarray]:
    """get_estimated_control_group_param (run_inference_two_groups.py:76-89):
    returns (log P_ctrl [K,K] with -inf diagonal, omega_logit_control [K])."""
    p = np.zeros((K, K))
    i = 0
    for r in range(K):
        for r1 in range(K):
            if r != r1:
                p[r, r1] = math.exp(theta[i])
                i += 1
        p[r, :] /= p[r, :].sum()
    with np.errstate(divide="ignore"):
        return np.log(p), np.asarray(theta[-K:], dtype=np.float64)


def uniform_theta(K: int, omega: float = 0.8) -> np.ndarray:
    return np.concatenate([np.zeros(K * (K - 1)), np.full(K, math.log(omega / (1.0 - omega)))])


class CaseControlModel:
    """Parameters of CaseControlRegimeModel + the proposal sizes, as a C-ABI model."""

    def __init__(self, mu: Sequence[float], sigma: Sequence[float], theta: Sequence[float],
                 minimum_duration: int = 3, omega_case: float = 0.8, merge_log_prob: float = math.log(0.1),
                 split_prob: float = 0.01, num_resampled_ancestors: int = 50, num_samples_backward: int = 25,
                 kappa_control: float = 2.0, kappa_case: float = 2.0, max_total_reads: int = 1023,
                 max_duration: int = 110000, optimal_resampling: bool = True, multinomial: bool = False):
        self.params = _lib.make_params(mu, sigma, theta, minimum_duration, num_resampled_ancestors,
                                       num_samples_backward, omega_case, merge_log_prob, split_prob,
                                       kappa_control, kappa_case, optimal_resampling, multinomial)
        self.n_regimes = len(mu)
        self.num_resampled_ancestors = int(num_resampled_ancestors)
        self.num_samples_backward = int(num_samples_backward)
        self.max_total_reads = int(max_total_reads)
        self.max_duration = int(max_duration)
        L = _lib.load()
        h = C.c_void_p()
        _lib.check(L.hyg_tg_model_create(C.byref(self.params), self.max_total_reads, self.max_duration, C.byref(h)))
        self._h = h

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    @property
    def num_particles(self) -> int:
        """N_max = M (2K + K^2) (run_inference_two_groups.py:263)."""
        return int(_lib.load().hyg_tg_num_particles(self._h))

    @property
    def global_weights(self) -> bool:
        """Whether the chains keep their particle arrays in global memory (the
        shapes whose N_max log-weights and sort keys exceed the LDS of a CU)."""
        return bool(_lib.load().hyg_tg_global_weights(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().hyg_tg_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _handle_array(models):
    return (C.c_void_p * len(models))(*[m.handle for m in models])


def _models_of(model, chain_model, n_chains: int):
    """A launch's models, resolved once: (models, handle array, index). One
    CaseControlModel: its handle and no index (the single-model entry points
    and their kernels). A list of models that share a launch
    (hyg_tg_models_compatible) with chain_model: the per-chain int32 index into
    it (the _multi entry points, also for a list of one)."""
    if isinstance(model, CaseControlModel):
        if chain_model is not None:
            raise ValueError("chain_model needs a list of models")
        return [model], _handle_array([model]), None
    models = list(model)
    if not models or chain_model is None:
        raise ValueError("a list of models needs a per-chain model index (chain_model)")
    idx = np.ascontiguousarray(chain_model, dtype=np.int32)
    if idx.shape != (n_chains,):
        raise ValueError(f"chain_model must have one index per chain ({n_chains})")
    if idx.min(initial=0) < 0 or idx.max(initial=0) >= len(models):
        raise ValueError(f"chain_model index out of [0, {len(models)})")
    handles = _handle_array(models)
    _lib.check(_lib.load().hyg_tg_models_compatible(handles, len(models)))
    return models, handles, idx


def _entry(name: str, handles, multi: bool):
    """The C entry `name` of a launch and its leading model arguments: the
    single-model one with the one handle, or `name`_multi with the handle
    array. A single-model launch never goes through a _multi entry: those run
    other kernel builds."""
    L = _lib.load()
    return (getattr(L, name + "_multi"), (handles, len(handles))) if multi else (getattr(L, name), (handles[0],))


def _index_args(idx) -> tuple:
    """The per-chain model index argument of a _multi entry (none for a single-model one)."""
    return () if idx is None else (idx.ctypes.data_as(C.POINTER(C.c_int32)),)


def genome_models(thetas: Sequence[Sequence[float]], mu: Sequence[float], sigma: Sequence[float],
                  max_total_reads: int, max_durations: Sequence[int], **kw) -> List[CaseControlModel]:
    """The models of a genome, one per theta (theta_{chrom}.csv.gz differs from
    chromosome to chromosome), built with one common max_total_reads so that
    one emission table serves every chain of a multi-model launch; each model
    keeps its own max_duration. kw: CaseControlModel's other parameters."""
    if len(thetas) != len(max_durations):
        raise ValueError("one max_duration per theta")
    models: List[CaseControlModel] = []
    try:
        for theta, md in zip(thetas, max_durations):
            models.append(CaseControlModel(mu, sigma, theta, max_total_reads=int(max_total_reads),
                                           max_duration=int(md), **kw))
    except BaseException:
        for m in models:
            m.close()
        raise
    return models


def _counts(meth_c, tot_c, meth_k, tot_k):
    """The four count matrices of a launch as contiguous uint16 [T, S] arrays."""
    out = []
    for a in (meth_c, tot_c, meth_k, tot_k):
        a = np.asarray(a)
        if a.ndim == 1:
            a = a[:, None]
        if np.any(a < 0) or np.any(a > 65535) or np.any(np.floor(a) != a):
            raise ValueError("read counts must be integers in [0, 65535]")
        out.append(np.ascontiguousarray(a, dtype=np.uint16))
    mc, tc, mk, tk = out
    if mc.shape != tc.shape or mk.shape != tk.shape or tk.shape[0] != tc.shape[0]:
        raise ValueError("inconsistent count shapes")
    return mc, tc, mk, tk


def _chain_array(chains):
    """The TgChain array of (site_begin, n_sites, seed, chain_id, out_begin) tuples."""
    arr = (_lib.TgChain * len(chains))()
    for i, (site_begin, n_sites, seed, chain_id, out_begin) in enumerate(chains):
        arr[i].site_begin, arr[i].n_sites = int(site_begin), int(n_sites)
        arr[i].seed, arr[i].chain_id, arr[i].out_begin = int(seed), int(chain_id), int(out_begin)
    return arr


def _host_outputs(K: int, B: int, n_rows: int, n_chains: int, n_particles: int = None) -> Dict[str, np.ndarray]:
    """The host output arrays of a launch (final_w with n_particles only)."""
    R, n = int(n_rows), int(n_chains)
    out = {"merged": np.empty((R, B), np.int16), "control": np.empty((R, B, 2), np.int16),
           "case": np.empty((R, B, 2), np.int16), "split_probs": np.empty(R, np.float32),
           "regime_probs": np.empty((R, 2 * K), np.float32), "log_z": np.empty(n, np.float64),
           "status": np.empty(n, np.int32)}
    if n_particles is not None:
        out["final_w"] = np.empty((n, int(n_particles)), np.float64)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run_chains_host_rc(handles, idx, counts, arr, out) -> int:
    """The batched host entry on the pieces above: hyg_tg_run_chains_host for
    one handle and no index, else hyg_tg_run_chains_host_multi. Returns the
    entry's code (the chain server answers a failed launch per request)."""
    mc, tc, mk, tk = counts
    fn, head = _entry("hyg_tg_run_chains_host", handles, idx is not None)
    return fn(*head, _ptr(mc), _ptr(tc), mc.shape[1], _ptr(mk), _ptr(tk), mk.shape[1], tc.shape[0], arr,
              *_index_args(idx), len(arr), out["merged"].shape[0], _ptr(out["merged"]), _ptr(out["control"]),
              _ptr(out["case"]), _ptr(out["split_probs"]), _ptr(out["regime_probs"]), _ptr(out["log_z"]),
              _ptr(out.get("final_w")), _ptr(out["status"]))


def run(observations: Dict[str, np.ndarray], n_total_reads: Dict[str, np.ndarray], model: CaseControlModel,
        seed: int, chain_id: int = 0):
    """filter_and_smoother_algorithm.run for the CaseControlRegimeModel: particle
    filter with optimal finite-state resampling + backward simulation of
    num_samples_backward trajectories.

    observations / n_total_reads: {'control': [T,S_c], 'case': [T,S_k]} methylated
    and total read counts. Returns (BackwardSimulationResults, final weights
    [N_max], extras) with extras = {'split_probs', 'regime_probs', 'log_z'} the
    posterior means of run_inference_two_groups.py:233-240, 289-296.
    """
    mc, tc, mk, tk = _counts(observations["control"], n_total_reads["control"], observations["case"],
                             n_total_reads["case"])
    T = tc.shape[0]
    if T > model.max_duration:
        raise ValueError(f"{T} sites exceed the model's max_duration {model.max_duration}")
    out = _host_outputs(model.n_regimes, model.num_samples_backward, T, 1, model.num_particles)
    _lib.check(_lib.load().hyg_tg_run_chain_host(
        model.handle, _ptr(mc), _ptr(tc), mc.shape[1], _ptr(mk), _ptr(tk), mk.shape[1], T, int(seed), int(chain_id),
        _ptr(out["merged"]), _ptr(out["control"]), _ptr(out["case"]), _ptr(out["split_probs"]),
        _ptr(out["regime_probs"]), _ptr(out["log_z"]), _ptr(out["final_w"])))
    res = BackwardSimulationResults(step=np.arange(T), particle={
        "merged_state": out["merged"], "control_state": out["control"], "case_state": out["case"]})
    return res, out["final_w"][0], {"split_probs": out["split_probs"], "regime_probs": out["regime_probs"],
                                    "log_z": float(out["log_z"][0])}


def run_chains_host(observations: Dict[str, np.ndarray], n_total_reads: Dict[str, np.ndarray],
                    model, chains: List[Tuple[int, int, int, int, int]], n_out_rows: int,
                    final_weights: bool = False, chain_model=None) -> Dict[str, np.ndarray]:
    """Many chains in one launch from host arrays (hyg_tg_run_chains_host), with
    no torch: `hygeia infer_many`'s every (batch, seed) task of a chromosome.
    chains: (site_begin, n_sites, seed, chain_id, out_begin) over the count rows
    and the output rows. Returns host arrays: merged [R,B], control / case
    [R,B,2], split_probs [R], regime_probs [R,2K], log_z / status [n_chains]
    (and final_w [n_chains, N_max]); each chain's rows are those of run().

    model: one CaseControlModel, or a list of models that differ in theta (a
    genome's chromosomes; genome_models) with chain_model[i] the index of chain
    i's model: hyg_tg_run_chains_host_multi, still one launch, each chain's rows
    those of run() with its own model."""
    counts = _counts(observations["control"], n_total_reads["control"], observations["case"], n_total_reads["case"])
    if not chains:
        raise ValueError("no chains to run")
    n_rows = int(n_out_rows)
    spans = sorted((int(c[4]), int(c[4]) + int(c[1])) for c in chains)
    if spans[0][0] < 0 or spans[-1][1] > n_rows or any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        raise ValueError("chains' output rows [out_begin, out_begin + n_sites) must be disjoint and inside "
                         f"[0, {n_rows})")
    models, handles, idx = _models_of(model, chain_model, len(chains))
    if idx is not None:
        if any(int(c[1]) > models[int(k)].max_duration for c, k in zip(chains, idx)):
            raise ValueError("a chain exceeds its model's max_duration")
    elif max(int(c[1]) for c in chains) > model.max_duration:
        raise ValueError(f"a chain exceeds the model's max_duration {model.max_duration}")
    m0 = models[0]  # the shape the launch's models share
    out = _host_outputs(m0.n_regimes, m0.num_samples_backward, n_rows, len(chains),
                        m0.num_particles if final_weights else None)
    _lib.check(_run_chains_host_rc(handles, idx, counts, _chain_array(chains), out))
    return out


class DeviceChains:
    """Batched device-resident execution of many chains (the bench and the
    multi-chain driver): emission table, history workspace and outputs are
    torch tensors on the current HIP device; kernels go to `stream`.
    `workspace` (uint8 tensor) lets batches that run one after another on one
    stream share the forward->backward history buffer. `model` is one
    CaseControlModel or a list of models with `chain_model`, the per-chain
    index into it (run_chains_host): the emission table is formed with the
    first model, and run() is one multi-model launch."""

    @staticmethod
    def workspace_bytes(model, chains) -> int:
        multi = not isinstance(model, CaseControlModel)
        fn, head = _entry("hyg_tg_workspace_bytes", _handle_array(model if multi else [model]), multi)
        return int(fn(*head, len(chains), sum(int(c[1]) for c in chains)))

    def __init__(self, model, chains: List[Tuple[int, int, int, int, int]], n_out_rows: int,
                 device=None, final_weights: bool = False, workspace=None, chain_model=None):
        import torch

        if _lib.load() is not None and not _lib.loaded_with_torch():
            raise RuntimeError("the HIP library was loaded without torch (import_torch=False): torch's HIP "
                               "runtime must initialise first for device-tensor chains")

        self.torch = torch
        self.models, self._handles, self._idx = _models_of(model, chain_model, len(chains))
        self.ws_bytes = self.workspace_bytes(model, chains)
        self.model = model = self.models[0]  # the shared shape and emission table
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        K, B = model.n_regimes, model.num_samples_backward
        self.chains = chains
        self._arr = _chain_array(chains)
        fn, head = _entry("hyg_tg_run_chains", self._handles, self._idx is not None)
        self._launch = (fn, *head, self._arr, *_index_args(self._idx), len(chains))  # run()'s entry and first arguments
        dev = self.device
        if workspace is not None:  # shared with other DeviceChains run one after another on one stream
            if workspace.numel() < self.ws_bytes or workspace.dtype != torch.uint8:
                raise ValueError(f"workspace of {workspace.numel()} bytes < {self.ws_bytes} needed")
            self.ws = workspace
        else:
            self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.merged = torch.empty((n_out_rows, B), dtype=torch.int16, device=dev)
        self.control = torch.empty((n_out_rows, B, 2), dtype=torch.int16, device=dev)
        self.case = torch.empty((n_out_rows, B, 2), dtype=torch.int16, device=dev)
        self.split_probs = torch.empty(n_out_rows, dtype=torch.float32, device=dev)
        self.regime_probs = torch.empty((n_out_rows, 2 * K), dtype=torch.float32, device=dev)
        self.log_z = torch.empty(len(chains), dtype=torch.float64, device=dev)
        self.status = torch.zeros(len(chains), dtype=torch.int32, device=dev)
        self.final_w = (torch.empty((len(chains), model.num_particles), dtype=torch.float64, device=dev)
                        if final_weights else None)
        self._out = _lib.TgOutputs(self.merged.data_ptr(), self.control.data_ptr(), self.case.data_ptr(),
                                   self.split_probs.data_ptr(), self.regime_probs.data_ptr(), self.log_z.data_ptr(),
                                   self.final_w.data_ptr() if self.final_w is not None else None,
                                   self.status.data_ptr())

    def emission(self, meth_c, tot_c, meth_k, tot_k, E=None, stream=None):
        """Beta-Binomial emission table [n_sites, 2K] f64 from device uint16 counts."""
        torch = self.torch
        T = tot_c.shape[0]
        if E is None:
            E = torch.empty((T, 2 * self.model.n_regimes), dtype=torch.float64, device=self.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.load().hyg_tg_emission(self.model.handle, meth_c.data_ptr(), tot_c.data_ptr(),
                                               tot_c.shape[1], meth_k.data_ptr(), tot_k.data_ptr(), tot_k.shape[1],
                                               T, E.data_ptr(), C.c_void_p(s)))
        return E

    def run(self, E, stream=None) -> None:
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device).cuda_stream
        fn, *head = self._launch
        _lib.check(fn(*head, E.data_ptr(), self.ws.data_ptr(), self.ws_bytes, C.byref(self._out), C.c_void_p(s)))


def _check_durations(model, models, idx, chains) -> None:
    if idx is not None:
        if any(int(c[1]) > models[int(k)].max_duration for c, k in zip(chains, idx)):
            raise ValueError("a chain exceeds its model's max_duration")
    elif max(int(c[1]) for c in chains) > model.max_duration:
        raise ValueError(f"a chain exceeds the model's max_duration {model.max_duration}")


TRACES = (None, "log_z", "all")  # the trace keyword of filter_chains_host / DeviceFilter


def _trace_rows(trace, chains, n_out_rows) -> int:
    """The rows of a traced launch's per-site arrays: n_out_rows, inside which
    the chains' rows [out_begin, out_begin + n_sites) are disjoint."""
    if trace not in TRACES:
        raise ValueError(f"trace must be one of {TRACES}, not {trace!r}")
    if trace is None:
        if n_out_rows is not None:
            raise ValueError("n_out_rows goes with a trace")
        return 0
    if n_out_rows is None:
        raise ValueError("a traced launch needs n_out_rows")
    n_rows = int(n_out_rows)
    spans = sorted((int(c[4]), int(c[4]) + int(c[1])) for c in chains)
    if spans[0][0] < 0 or spans[-1][1] > n_rows or any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        raise ValueError("chains' output rows [out_begin, out_begin + n_sites) must be disjoint and inside "
                         f"[0, {n_rows})")
    return n_rows


def filter_chains_host(observations: Dict[str, np.ndarray], n_total_reads: Dict[str, np.ndarray], model,
                       chains: List[Tuple[int, int, int, int, int]], final_weights: bool = False,
                       chain_model=None, trace=None, n_out_rows=None) -> Dict[str, np.ndarray]:
    """The particle filter of many chains in one forward-only launch from host
    arrays (hyg_tg_filter_chains_host[_multi]), with no torch: log Z, the
    estimate of the marginal likelihood, without ancestor history, backward
    simulation or trajectories. chains, model and chain_model as
    run_chains_host (a chain's out_begin is ignored). Returns host arrays
    log_z / status [n_chains] (and final_w [n_chains, N_max]), each chain's bit
    for bit those of run_chains_host.

    trace="log_z" or "all": the traced launch (hyg_tg_trace_chains_host[_multi]),
    which honours out_begin over n_out_rows rows and also returns log_z_t
    [n_out_rows] f64, row out_begin + t the log Z of the chain's first t + 1
    sites, and for "all" the filtering marginals split_probs [n_out_rows] and
    regime_probs [n_out_rows, 2K] f32 (include/hygeia_amd.h). Rows no chain owns
    hold NaN."""
    counts = _counts(observations["control"], n_total_reads["control"], observations["case"], n_total_reads["case"])
    if not chains:
        raise ValueError("no chains to run")
    n_rows = _trace_rows(trace, chains, n_out_rows)
    models, handles, idx = _models_of(model, chain_model, len(chains))
    _check_durations(model, models, idx, chains)
    n = len(chains)
    out = {"log_z": np.empty(n, np.float64), "status": np.empty(n, np.int32)}
    if final_weights:
        out["final_w"] = np.empty((n, models[0].num_particles), np.float64)
    mc, tc, mk, tk = counts
    if trace is not None:
        out["log_z_t"] = np.full(n_rows, np.nan, np.float64)
        if trace == "all":
            out["split_probs"] = np.full(n_rows, np.nan, np.float32)
            out["regime_probs"] = np.full((n_rows, 2 * models[0].n_regimes), np.nan, np.float32)
        fn, head = _entry("hyg_tg_trace_chains_host", handles, idx is not None)
        _lib.check(fn(*head, _ptr(mc), _ptr(tc), mc.shape[1], _ptr(mk), _ptr(tk), mk.shape[1], tc.shape[0],
                      _chain_array(chains), *_index_args(idx), n, n_rows, _ptr(out["log_z_t"]),
                      _ptr(out.get("split_probs")), _ptr(out.get("regime_probs")), _ptr(out["log_z"]),
                      _ptr(out.get("final_w")), _ptr(out["status"])))
        return out
    fn, head = _entry("hyg_tg_filter_chains_host", handles, idx is not None)
    _lib.check(fn(*head, _ptr(mc), _ptr(tc), mc.shape[1], _ptr(mk), _ptr(tk), mk.shape[1], tc.shape[0],
                  _chain_array(chains), *_index_args(idx), n, _ptr(out["log_z"]), _ptr(out.get("final_w")),
                  _ptr(out["status"])))
    return out


class DeviceFilter:
    """Device-resident forward-only launches (benchmarks): model, chains and
    chain_model as DeviceChains. Allocates only the filter workspace (no
    history), log_z, status and, with final_weights, final_w; the emission
    table comes from a DeviceChains.emission or from emission() here. With
    trace="log_z" or "all" (filter_chains_host) the launch is the traced one
    (hyg_tg_trace_chains[_multi]) over n_out_rows rows: log_z_t and, for "all",
    split_probs and regime_probs."""

    @staticmethod
    def workspace_bytes(model, chains) -> int:
        multi = not isinstance(model, CaseControlModel)
        fn, head = _entry("hyg_tg_filter_workspace_bytes", _handle_array(model if multi else [model]), multi)
        return int(fn(*head, len(chains)))

    def __init__(self, model, chains: List[Tuple[int, int, int, int, int]], device=None,
                 final_weights: bool = False, chain_model=None, trace=None, n_out_rows=None):
        import torch

        if _lib.load() is not None and not _lib.loaded_with_torch():
            raise RuntimeError("the HIP library was loaded without torch (import_torch=False): torch's HIP "
                               "runtime must initialise first for device-tensor chains")
        self.torch = torch
        n_rows = _trace_rows(trace, chains, n_out_rows)
        self.models, self._handles, self._idx = _models_of(model, chain_model, len(chains))
        self.ws_bytes = self.workspace_bytes(model, chains)
        self.model = model = self.models[0]  # the shared shape and emission table
        self.device = dev = device or torch.device("cuda", torch.cuda.current_device())
        self.chains = chains
        self._arr = _chain_array(chains)
        self.trace = trace
        fn, head = _entry("hyg_tg_trace_chains" if trace else "hyg_tg_filter_chains", self._handles,
                          self._idx is not None)
        self._launch = (fn, *head, self._arr, *_index_args(self._idx), len(chains))
        self.ws = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=dev)
        self.log_z = torch.empty(len(chains), dtype=torch.float64, device=dev)
        self.status = torch.zeros(len(chains), dtype=torch.int32, device=dev)
        self.final_w = (torch.empty((len(chains), model.num_particles), dtype=torch.float64, device=dev)
                        if final_weights else None)
        self._trace = None
        if trace:
            self.log_z_t = torch.full((n_rows,), float("nan"), dtype=torch.float64, device=dev)
            self.split_probs = self.regime_probs = None
            if trace == "all":
                self.split_probs = torch.full((n_rows,), float("nan"), dtype=torch.float32, device=dev)
                self.regime_probs = torch.full((n_rows, 2 * model.n_regimes), float("nan"), dtype=torch.float32,
                                               device=dev)
            self._trace = _lib.TgTrace(self.log_z_t.data_ptr(),
                                       self.split_probs.data_ptr() if trace == "all" else None,
                                       self.regime_probs.data_ptr() if trace == "all" else None)

    emission = DeviceChains.emission

    def run(self, E, stream=None) -> None:
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device).cuda_stream
        fn, *head = self._launch
        trace = (C.byref(self._trace),) if self._trace is not None else ()
        _lib.check(fn(*head, E.data_ptr(), self.ws.data_ptr(), self.ws_bytes, *trace, self.log_z.data_ptr(),
                      self.final_w.data_ptr() if self.final_w is not None else None, self.status.data_ptr(),
                      C.c_void_p(s)))
