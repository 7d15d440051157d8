"""SparseGPT local pruning driven by the ECoFLaP sparsity table.

Host-side mirror of LAVIS/lavis/compression/pruners/sparsegpt_pruner.py:
  SparseGPT (:56-222): Hessian accumulation, damped Cholesky x2, blockwise OBS sweep
  T5 / VIT / BLIPT5 LayerSparseGPTPruner (:226-963): same block-sequential loop as the Wanda
  pruners with SparseGPT in place of WrappedGPT; registered names kept.

The Hessian update of fp16 / bf16 activations is a hand-written MFMA SYRK
(`ecoflap_hessian_accum`, csrc/syrk.hip; fp32 activations and the trailing update are plain
library GEMMs, torch.addmm -> hipBLASLt); the two damped Cholesky factorisations and the
inverse from the factor are the build's own fp32 kernels (csrc/cholesky.hip; torch.linalg's
with `SparseGPT.use_own_cholesky = False`); the per-block threshold + sequential sweep, which
torch runs as ~1000 small kernels per 128 columns, is one fused HIP step
(`ecoflap_sparsegpt_block`, csrc/sparsegpt.hip).  With `SparseGPT.whole_matrix_sweep` (off by
default; `clip_sparsegpt_pruner` turns it on) the whole sweep of a Linear — the fp32 copy, every
block step, every trailing update on an fp32 MFMA kernel of the build, the cast back — is ONE host
call (`ecoflap_sparsegpt_matrix`), and `SparseGPT.sweep_group` sweeps Linears that share one factor
(twins: the same input) side by side in one call (`ecoflap_sparsegpt_matrix_group`;
`llama_sparsegpt_pruner`).
"""
import math

import torch
import torch.nn as nn

from .. import hip as _hip
from ..registry import registry
from .phase_timer import PhaseTimer
from .wanda import BLIPT5LayerWandaPruner, T5LayerWandaPruner, VITLayerWandaPruner


class SparseGPT:
    use_mfma_hessian = True     # False: the reference's fp32 expression through the library GEMM
    # MFMA path: calibration samples whose inputs are reduced in ONE call.  The reference's
    # per-sample recurrence (:71-82) unrolls to H_J = (n_0 / n_J) H_0 + (2 / n_J) sum_j X_j^T X_j,
    # i.e. one update with the samples' tokens concatenated: H (151 MB at 6144 columns) is read
    # and written once per `samples_per_call` samples instead of once per sample.
    samples_per_call = 8

    def __init__(self, layer, kernels=None):
        self.layer = layer
        self.dev = self.layer.weight.device
        W = layer.weight.data
        assert isinstance(layer, nn.Linear), "the path only prunes nn.Linear"
        self.rows = W.shape[0]
        self.columns = W.shape[1]
        self.H = torch.zeros((self.columns, self.columns), device=self.dev)
        self.nsamples = 0
        self.factor = None          # (dead columns, Hinv) once pruned; shared within a block
        self.kernels = kernels if kernels is not None else _hip.HipKernels()
        self._pending = []          # (x [tokens, cols], batch) waiting for one MFMA call

    def add_batch(self, inp, out):
        """H <- H * n/(n+b) + (sqrt(2/(n+b)) x)^T (sqrt(2/(n+b)) x)   (:71-82)"""
        if len(inp.shape) == 2:
            inp = inp.unsqueeze(0)
        self.add_rows(inp.reshape((-1, inp.shape[-1])), inp.shape[0])

    def add_rows(self, x, tmp):
        """`add_batch` for rows already flattened to [tokens, columns], in any order (a Hessian is a
        sum over rows), counted as `tmp` samples."""
        if (self.use_mfma_hessian and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16)
                and hasattr(self.kernels, "hessian_accum")):
            # fp16 / bf16 activations (the forward under autocast): beta*H + alpha*x^T x on the
            # matrix cores, upper triangle once (csrc/syrk.hip), several samples per call
            # (held as it is, not cloned, until the buffer is flushed: an op that writes this Linear's
            # input in place later in the forward would change H silently — checked at the flush)
            xc = x if x.is_contiguous() else x.contiguous()
            self._pending.append((xc, tmp, xc._version))
            if len(self._pending) >= self.samples_per_call:
                self.flush()
            return
        self.flush()
        self.H *= self.nsamples / (self.nsamples + tmp)
        self.nsamples += tmp
        xs = math.sqrt(2 / self.nsamples) * x.float()
        if self.literal_update:
            self.H += xs.t().matmul(xs)
        else:
            self.H.addmm_(xs.t(), xs)

    # The fp32 update as the reference writes it, `H += inp.matmul(inp.t())`: the product rounded on
    # its own, then added.  `addmm_` hands H to the GEMM as its accumulator, and a library that
    # blocks over k then rounds in another order (a CPU GEMM does above a few hundred tokens).
    # The pruners that came first keep `addmm_` and their recorded hashes; `clip_sparsegpt_pruner`
    # and `llama_sparsegpt_pruner` set this on their own objects.
    literal_update = False

    def flush(self):
        """Reduce the buffered samples into H (called when the buffer is full and before H is
        read: merge across ranks, twin detection, `fasterprune`)."""
        if not self._pending:
            return
        for x, _, version in self._pending:
            if x._version != version:
                self._pending = []
                raise RuntimeError(
                    "SparseGPT: a hooked Linear input was modified in place after the hook saw it "
                    "(the reference reduces it inside the hook, sparsegpt_pruner.py:71-82); set "
                    "SparseGPT.samples_per_call = 1 for a model that writes activations in place")
        xs = [x for x, _, _ in self._pending]
        b = sum(n for _, n, _ in self._pending)
        self._pending = []
        with PhaseTimer.span("sparsegpt.hessian (cat + MFMA SYRK)"):
            x = xs[0] if len(xs) == 1 else torch.cat(xs, 0)
            self.kernels.hessian_accum(self.H, x, self.nsamples, b)
        self.nsamples += b

    # The reference's expression as it stands: torch.quantile takes at most 2^24 elements, so above
    # 4096 columns a Hessian that holds an inf raises here, as it does in the reference.
    @staticmethod
    def _clamp_inf(H):
        if (torch.isinf(H) * (H > 0)).float().sum() > 0:          # (:104-112, :136-144)
            H[torch.isinf(H) * (H > 0)] = torch.quantile(H, 0.999)
        if (torch.isinf(H) * (H < 0)).float().sum() > 0:
            H[torch.isinf(H) * (H < 0)] = torch.quantile(H, 0.001)

    # The two Cholesky factorisations by this build's own blocked fp32 kernel (csrc/cholesky.hip,
    # round 6) where the backend has one: rocSOLVER's potrf is latency-bound at these sizes (4-20 ms
    # where the flops are worth 0.1-1.5) and not safe with two calls in flight.  Against the fp64
    # result, up to n = 6144: the factor is within 3-5e-7 of its scale and the inverse within
    # 6-9e-7 (the library: 4-6e-7 and 0.6-1.2e-6; the inverse's long sums are compensated, see
    # cholesky.hip), not bit for bit the library's — fp32 factorisations re-associate: the tests
    # that hold the HIP backend to the oracle backend BIT FOR BIT switch this off so that both
    # sides factor with the same library call (as they do for `use_mfma_hessian`).
    use_own_cholesky = True

    def _cholesky_inverse(self, L):
        if (self.use_own_cholesky and L.is_cuda and L.dtype == torch.float32
                and hasattr(self.kernels, "cholesky_inverse")):
            return self.kernels.cholesky_inverse(L)
        return torch.cholesky_inverse(L)

    def _damped_cholesky(self, H, damp, upper):
        diag = torch.arange(H.shape[0], device=H.device)
        own = (self.use_own_cholesky and H.is_cuda and H.dtype == torch.float32
               and hasattr(self.kernels, "cholesky"))
        for _ in range(10000):                                    # the reference loops forever
            if own:
                # (a NaN anywhere in the lower triangle reaches a pivot and is reported there)
                L, info = self.kernels.cholesky(H, upper=upper)
                if info == 0:
                    return L
            else:
                L, info = torch.linalg.cholesky_ex(H, upper=upper)
                if int(info) == 0 and not torch.isnan(L).any():
                    return L
            H[diag, diag] += damp                                 # not positive definite yet
        raise RuntimeError("Hessian could not be made positive definite")

    # ---- the factorisations of a block's Linears ---------------------------------------------------
    _pool = None
    _pool_streams = {}

    def _own_factorisations(self):
        return (self.use_own_cholesky and self.H is not None and self.H.is_cuda and self.H.dtype == torch.float32
                and hasattr(self.kernels, "cholesky") and hasattr(self.kernels, "cholesky_inverse"))

    @classmethod
    def factor_all(cls, items, percdamp=.01):
        """`factor` (dead columns, Hinv) for every SparseGPT in `items` — the three factorisation
        calls of `fasterprune` (:84-110) — up front for a whole transformer block.

        History.  Round 5 ran them side by side on rocSOLVER (latency-bound at these sizes: 4.0 ms
        at 1408, 20 ms at 6144; a block's Hessians are independent), one host thread + stream +
        solver handle per Linear — and withdrew it: `tools/diag/factor_determinism.py` showed 4-8
        corrupted factors (1e-4 .. 1e-2, not rounding) per 400 side-by-side factorisations against
        0 in 160 one-by-one, with locks around the Cholesky calls alone and around the inverse
        alone as well: two solver calls in flight in one process are not safe on this stack
        (`profiles/r05_sparsegpt/README.md`).

        Round 6: the factorisations are this build's own kernels (csrc/cholesky.hip: no solver
        handle, no workspace outside the call; 10.2 -> 2.8 s of the BLIP-2 run's stage 2 one by
        one), and with THOSE the side-by-side form is back: one host thread and one HIP stream per
        Linear, each running exactly `_factor_alone` — the reference's sequence with its own
        host-side tests (`info`, the inf scans), which then wait on that thread's stream only —
        so every factor is the one-by-one factor bit for bit (the same probe: 0 of 400;
        tests/test_sparsegpt_parity.py).  A backend without the own kernels (the oracle backend,
        `use_own_cholesky = False`) factors one at a time on the caller's stream, as before."""
        items = [it for it in items if it.factor is None]
        if not items:
            return
        for it in items:
            it.flush()
        if not (len(items) > 1 and cls.side_by_side and all(it._own_factorisations() for it in items)):
            for it in items:
                it._factor_alone(percdamp)
            return
        import concurrent.futures as cf
        import threading
        if cls._pool is None:
            cls._pool = cf.ThreadPoolExecutor(max_workers=8, thread_name_prefix="sparsegpt-factor")
        main = torch.cuda.current_stream()
        device = torch.cuda.current_device()
        done_streams = []

        def work(it):
            torch.cuda.set_device(device)
            tid = threading.get_ident()
            st = cls._pool_streams.get((tid, device))
            if st is None:
                st = cls._pool_streams[(tid, device)] = torch.cuda.Stream()
            st.wait_stream(main)
            with torch.cuda.stream(st), torch.no_grad():
                it._factor_alone(percdamp)
                st.synchronize()
            done_streams.append(st)

        # (largest first: the block's 5120 / 6144 Hessian is the critical path)
        order = sorted(items, key=lambda it: -it.columns)
        for f in [cls._pool.submit(work, it) for it in order]:
            f.result()
        for st in done_streams:
            main.wait_stream(st)
        for it in items:
            for t in it.factor:          # made on a side stream, read by the sweep on this one
                t.record_stream(main)

    side_by_side = True

    def _factor_alone(self, percdamp):
        H = self.H
        dead = torch.diag(H) == 0
        H[dead, dead] = 1
        self._clamp_inf(H)
        damp = percdamp * torch.mean(torch.diag(H))
        H = self._damped_cholesky(H, damp, upper=False)
        H = self._cholesky_inverse(H)
        self._clamp_inf(H)
        damp = percdamp * torch.mean(torch.diag(H).abs())
        self.factor = (dead, self._damped_cholesky(H, damp, upper=True).contiguous())
        self.H = None

    # The column sweep of a Linear from ONE host call (`ecoflap_sparsegpt_matrix`: the fp32 copy,
    # every block step, every trailing update on this build's own MFMA kernel, the cast back) where
    # the backend has the entry and the weight is on the GPU.  Off by default: the trailing update
    # is then the library GEMM, whose roundings the pruners' recorded hashes hold;
    # `clip_sparsegpt_pruner` turns it on for its own objects.
    whole_matrix_sweep = False

    def _one_call_sweep_applies(self, blocksize):
        w = self.layer.weight.data
        return (self.whole_matrix_sweep and w.is_cuda and w.dim() == 2 and w.is_contiguous()
                and 0 < blocksize <= 128 and hasattr(self.kernels, "sparsegpt_matrix"))

    def _sweep_in_one_call(self, sparsity, prune_n, prune_m, blocksize):
        dead, Hinv = self.factor
        ranks = None
        if prune_n == 0:                                   # int(tmp.numel() * sparsity) (:187)
            ranks = [int(self.rows * (min(i1 + blocksize, self.columns) - i1) * sparsity)
                     for i1 in range(0, self.columns, blocksize)]
        with PhaseTimer.span("sparsegpt.sweep (one call: csrc/sparsegpt.hip)"):
            self.kernels.sparsegpt_matrix(self.layer.weight.data, Hinv, dead, blocksize, ranks, prune_n, prune_m)

    @classmethod
    def sweep_group(cls, objects, sparsities, prune_n=0, prune_m=0, blocksize=128, percdamp=.01):
        """`fasterprune` of Linears that saw the very same inputs (q / k / v, gate / up: bit-identical
        H, checked by the caller), each at its own sparsity, sharing the factor of `objects[0]`.
        Where the one-call sweep applies to all of them and their weights have one dtype, column
        count and device, the sweeps run side by side in ONE host call
        (`ecoflap_sparsegpt_matrix_group`: per column block the launches of one matrix, every weight
        with the bits of its own sweep) -> True; otherwise one `fasterprune` each -> False."""
        first = objects[0]
        w0 = first.layer.weight.data
        grouped = (1 < len(objects) <= _hip.SGPT_MAX_GROUP
                   and hasattr(first.kernels, "sparsegpt_matrix_group")
                   and all(o._one_call_sweep_applies(blocksize) and o.kernels is first.kernels
                           and o.layer.weight.data.dtype == w0.dtype and o.columns == first.columns
                           and o.layer.weight.data.device == w0.device for o in objects))
        if not grouped:
            for i, (o, sparsity) in enumerate(zip(objects, sparsities)):
                o.fasterprune(sparsity, prune_n=prune_n, prune_m=prune_m, blocksize=blocksize, percdamp=percdamp,
                              same_hessian_as=first if i else None)
            return False
        for o in objects:
            o.flush()
        if first.factor is None:
            with PhaseTimer.span("sparsegpt.factor (clamp, 2 damped Cholesky, inverse: csrc/cholesky.hip)"):
                first._factor_alone(percdamp)
        dead, Hinv = first.factor
        ranks = None
        if prune_n == 0:                                   # int(tmp.numel() * sparsity) (:187), per member
            ranks = [[int(o.rows * (min(i1 + blocksize, o.columns) - i1) * sparsity)
                      for i1 in range(0, o.columns, blocksize)] for o, sparsity in zip(objects, sparsities)]
        for o in objects:
            o.H = None
            o.factor = first.factor
        with PhaseTimer.span("sparsegpt.sweep (one call per twin set: csrc/sparsegpt.hip)"):
            first.kernels.sparsegpt_matrix_group([o.layer.weight.data for o in objects], Hinv, dead, blocksize,
                                                 ranks, prune_n, prune_m)
        return True

    def fasterprune(self, sparsity, prune_n=0, prune_m=0, blocksize=128, percdamp=.01,
                    same_hessian_as=None):
        """`same_hessian_as`: a SparseGPT of this block that saw the very same inputs (q/k/v,
        wi_0/wi_1, cross-attention k/v: bit-identical H, checked by the caller) and has already
        been pruned — its dead-column mask and factor Hinv depend on H only and are reused
        instead of being recomputed (two Cholesky factorisations and an inverse each)."""
        self.flush()
        if self._one_call_sweep_applies(blocksize):
            src = self if same_hessian_as is None or same_hessian_as.factor is None else same_hessian_as
            if src.factor is None:
                with PhaseTimer.span("sparsegpt.factor (clamp, 2 damped Cholesky, inverse: csrc/cholesky.hip)"):
                    self._factor_alone(percdamp)
            self.H = None
            self.factor = src.factor
            self._sweep_in_one_call(sparsity, prune_n, prune_m, blocksize)
            return
        W = self.layer.weight.data.clone().float()
        H = self.H
        self.H = None
        if same_hessian_as is not None and same_hessian_as.factor is not None:
            dead, Hinv = same_hessian_as.factor
            W[:, dead] = 0
            del H
        elif self.factor is not None:               # factored with its block (`factor_all`)
            dead, Hinv = self.factor
            W[:, dead] = 0
        else:
            with PhaseTimer.span("sparsegpt.factor (clamp, 2 damped Cholesky, inverse: csrc/cholesky.hip)"):
                dead = torch.diag(H) == 0
                H[dead, dead] = 1
                W[:, dead] = 0
                with PhaseTimer.span("sparsegpt.factor.clamp_inf (isinf scans + host syncs)"):
                    self._clamp_inf(H)
                damp = percdamp * torch.mean(torch.diag(H))
                with PhaseTimer.span("sparsegpt.factor.cholesky_lower"):
                    H = self._damped_cholesky(H, damp, upper=False)
                with PhaseTimer.span("sparsegpt.factor.cholesky_inverse"):
                    H = self._cholesky_inverse(H)
                with PhaseTimer.span("sparsegpt.factor.clamp_inf (isinf scans + host syncs)"):
                    self._clamp_inf(H)
                damp = percdamp * torch.mean(torch.diag(H).abs())
                with PhaseTimer.span("sparsegpt.factor.cholesky_upper"):
                    Hinv = self._damped_cholesky(H, damp, upper=True).contiguous()
        self.factor = (dead, Hinv)
        with PhaseTimer.span("sparsegpt.sweep (threshold + OBS kernels + trailing GEMMs)"):
            for i1 in range(0, self.columns, blocksize):
                i2 = min(i1 + blocksize, self.columns)
                count = i2 - i1
                err = torch.empty((self.rows, count), dtype=torch.float32, device=W.device)
                with PhaseTimer.span("sparsegpt.sweep.block_kernels"):
                    if prune_n != 0:                              # n:m, mask grown in the sweep (:190, :196-198)
                        self.kernels.sparsegpt_block_nm(W, Hinv, i1, count, prune_n, prune_m, err)
                    else:
                        k = int(self.rows * count * sparsity)     # int(tmp.numel() * sparsity) (:187)
                        self.kernels.sparsegpt_block(W, Hinv, i1, count, k, err)
                if i2 < self.columns:
                    with PhaseTimer.span("sparsegpt.sweep.trailing_gemm"):
                        W[:, i2:] -= err.matmul(Hinv[i1:i2, i2:])     # (:216)
        self.layer.weight.data = W.reshape(self.layer.weight.shape).to(self.layer.weight.data.dtype)

    def free(self):
        self.H = None
        self.factor = None
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


@registry.register_pruner("t5_sparsegpt_pruner")
class T5LayerSparseGPTPruner(T5LayerWandaPruner):
    pruner_name = "t5_sparsegpt_pruner"
    local_method = "sparsegpt"


@registry.register_pruner("vit_sparsegpt_pruner")
class VITLayerSparseGPTPruner(VITLayerWandaPruner):
    pruner_name = "vit_sparsegpt_pruner"
    local_method = "sparsegpt"


@registry.register_pruner("blipt5_sparsegpt_pruner")
class BLIPT5LayerSparseGPTPruner(BLIPT5LayerWandaPruner):
    pruner_name = "blipt5_sparsegpt_pruner"
    local_method = "sparsegpt"
