"""Batch inference behind the reference's API (predict.py:45-96): run the tower
forward over an [N,F] feature array in chunks and return float32 [N,D].

The reference restores a TF checkpoint or reuses the live session
(``Prediction(sess=sess)``, train.py:282); here ``Prediction`` wraps the live
``VNetParams`` (or a checkpoint written by ``train.Trainer``).  Forward only:
l2norm -> FC -> FC -> l2norm, the same HIP kernels as training.
"""
import os

import numpy as np
import torch

from . import engine, ops


class Prediction():
    def __init__(self, params=None, ckpt=None, device="cuda:0", precision="f32", fc2_single_pass=False):
        """``precision``: "f32" (the reference's arithmetic), "f32x3" / "f16x2" (plane kernels) or "bf16" -- BASELINE config 4's
        precision for catalogue inference: an fp16 ``FeatureTableF16`` (or an fp8 ``FeatureTableF8``) in, bf16 MFMA projection,
        fp32 accumulation and output normalisation (build-defined; tolerance 5e-3 on the unit-norm
        embeddings, tests/test_gpu_bf16.py).  ``fc2_single_pass`` (precision "f32x3"): see
        engine_x3.TowerWorkspaceX3 -- off, an embedding's bits do not depend on the chunk size."""
        if params is None:
            if ckpt is None or not os.path.exists(ckpt):
                raise IOError("Prediction __init__ Cannot find %s" % ckpt)      # predict.py:54-55
            state = torch.load(ckpt, map_location="cpu")
        if precision not in ("f32", "bf16", "f32x3", "f16x2"):
            raise ValueError("precision must be 'f32', 'f32x3', 'f16x2' or 'bf16'")
        self.engine = engine.get_engine(precision)
        if params is None:
            params = engine.VNetParams(self.engine.layout(*state["layout"]), device)
            params.load(*[state["variables"][n] for n in engine.VNetParams.NAMES])
        # (live parameters may sit on a wider layout than the engine's own; the plane kernels need their tile's widths)
        L, w = params.layout, self.engine.Workspace.WIDTHS
        if L.Fp % w or L.Hp % w or L.Dp % w:
            raise ValueError("precision 'f32x3' needs parameters built on engine_x3.layout_x3 (widths padded to 256)")
        self.params = params
        self.device = params.device
        self.precision = precision
        self.fc2_single_pass = bool(fc2_single_pass)
        self._ws = None
        self._weights_fresh = False                      # embed_table: the operand copies are made once per pass

    def _workspace(self, n_rows):
        E = self.engine
        n_rows = engine.round_up(n_rows, E.rows)
        if self._ws is None or self._ws.R < n_rows:
            self._ws = E.workspace(self.params.layout, n_rows, self.device, backward=False, planes_in=False,
                                   fc2_single_pass=self.fc2_single_pass)
            if E.table_dtype == torch.float16:           # the fp16 catalogue's rows come through a gather (embed_table)
                self._ids = torch.arange(n_rows, dtype=torch.int32, device=self.device)
                self._idx = torch.zeros(n_rows, dtype=torch.int32, device=self.device)
        return self._ws

    def predict(self, input_batch):
        """input_batch: [n,F] ndarray / device tensor (raw features) or rows of a
        FeatureTable's padded storage.  Returns a device tensor [n,D]."""
        L, E = self.params.layout, self.engine
        if E.table_dtype == torch.float16:
            raise ValueError("bf16 inference reads an fp16 catalogue: use embed_table / run_features(FeatureTableF16)")
        x = input_batch if torch.is_tensor(input_batch) else torch.as_tensor(np.asarray(input_batch, np.float32))
        x = x.to(self.device, torch.float32)
        if x.stride(-1) != 1 or (x.stride(0) % 4) or (x.data_ptr() % 16):
            x = x.contiguous()
        n, most = x.shape[0], E.Workspace.MAX_ROWS
        if most and n > most:
            return torch.cat([self.predict(x[lo:lo + most]).clone() for lo in range(0, n, most)])
        ws = self._workspace(n)
        if L.F % 4:
            raise ValueError("feature size must be a multiple of 4")
        ops.l2norm_fwd(x[:, :L.F] if x.shape[1] != L.F else x, L.F, ws.x_hat)      # models.py:58
        if not self._weights_fresh:
            ws.observe_weights(self.params) or E.refresh_weights(self.params, ws)      # (f16x2: the scales, then the planes)
        # models.py:59-61 (the fp32 MFMA alone runs on part of a workspace: the others' row tiles take it whole)
        E.tower_forward(self.params, ws, **({"n_rows": n} if E.rows == 1 else {}))
        return ws.e[:n, :L.D]

    def embed_table(self, table, batch_size, out=None):
        """Embeddings of every row of a device-resident catalogue, ``batch_size`` rows at a time,
        into a DEVICE tensor [N, D] (predict.py:71-96 without its host round trip: the reference
        converts every chunk with ``.tolist()``, predict.py:79-86).  Enqueue-only."""
        L, N, E = self.params.layout, table.n_rows, self.engine
        if out is None:
            out = torch.empty((N, L.D), dtype=torch.float32, device=self.device)
        if E.table_dtype == torch.float16 and table.data.dtype not in E.table_dtypes:
            raise ValueError("precision 'bf16' reads an fp16 FeatureTableF16")
        if E.Workspace.MAX_ROWS:
            # h1 as three planes is 30 KB per row: the GEMMs' 2 GiB buffer descriptors take 65 536 rows at a time
            batch_size = min(batch_size, E.Workspace.MAX_ROWS)
        ws = self._workspace(min(batch_size, N))
        ws.observe_weights(self.params) or E.refresh_weights(self.params, ws)          # operand copies, once per pass
        if E.table_dtype == torch.float16:
            for lo in range(0, N, batch_size):
                n = min(batch_size, N - lo)
                torch.add(self._ids[:n], lo, out=self._idx[:n])
                gather = ops.gather_rows_f8 if table.data.dtype == torch.float8_e4m3fn else ops.gather_rows_f16
                gather(table.data, 0, self._idx[:n], table.feature_size, ws.x_hat)   # rows lo..lo+n, l2-normalised
                E.tower_forward(self.params, ws)
                out[lo:lo + n] = ws.e[:n, :L.D]
            return out
        feats = table.data[:, :table.feature_size] if table.data.shape[1] == table.feature_size else table.data
        self._weights_fresh = True
        try:
            for lo in range(0, N, batch_size):
                hi = min(lo + batch_size, N)
                out[lo:hi] = self.predict(feats[lo:hi])
        finally:
            self._weights_fresh = False
        return out

    def run_features(self, features, batch_size, output_dir='', suffix=''):
        """Embeddings of every row of ``features`` (ndarray, tensor or FeatureTable),
        ``batch_size`` rows at a time; float32 ndarray [N,D] like predict.py:71-96
        (saved to output_dir/output<suffix>.npy when output_dir is given)."""
        if isinstance(features, engine.FeatureTable):
            out = self.embed_table(features, batch_size)
        else:
            N = features.shape[0]
            out = torch.empty((N, self.params.layout.D), dtype=torch.float32, device=self.device)
            for lo in range(0, N, batch_size):
                hi = min(lo + batch_size, N)
                out[lo:hi] = self.predict(features[lo:hi])
        output_np = out.cpu().numpy()
        if output_dir:
            np.save(os.path.join(output_dir, "output" + suffix + ".npy"), output_np)
        return output_np
