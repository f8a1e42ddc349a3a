"""Device-resident gallery with exact inner-product top-k (libfrhip match kernel).

Drop-in for the reference's three match paths:
  * ``RecognitionEngine.recognize_with_db`` — per-row ``cosine_similarity`` loop + stable
    ``sort(reverse=True)`` (inference/recognition_engine.py:267-289, :41-63);
  * FAISS ``IndexFlatIP`` (``build_faiss_index`` extract_embeddings.py:595-645, searched in
    recognition_engine.py:291-326) — ``DeviceGallery`` exposes the same ``add``/``search``/
    ``ntotal`` surface, ``search`` returning (scores, ids) with ids int64 and -1 padding, plus
    ``range_search`` (score >= thresh, the reference's rule, where faiss is strict) and ``reconstruct_n``;
  * the notebook's batched ``np.dot(emb, P.T)`` + ``argmax``/``argsort[:, -5:]``.
Order is (score desc, index asc) everywhere, i.e. ``np.argmax``'s first-max rule and the
stable sort's insertion order on ties.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as N


class DeviceGallery:
    def __init__(self, rows=None, dim: int = 512, device: int = 0, index_base: int = 0, handle=None,
                 x3_min_rows: Optional[int] = None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("DeviceGallery needs a ROCm GPU; there is deliberately no CPU fallback")
        self.device = torch.device("cuda", device)
        self.d = dim
        self.index_base = int(index_base)
        self._own = handle is None
        if handle is None:
            h = ctypes.c_void_p()
            N.check(N.lib().fr_create(ctypes.byref(h), device, 0, N.FR_DTYPE_BF16), "fr_create")
            handle = h
        self._h = handle
        if x3_min_rows is not None:  # FR_OPT_X3_MIN_ROWS: smallest gallery given the bf16x3 path
            N.check(N.lib().fr_set_option(self._h, N.FR_OPT_X3_MIN_ROWS, int(x3_min_rows)), "fr_set_option")
        self._n = 0  # rows live on the device only (fr_gallery_write appends in place)
        N.check(N.lib().fr_gallery_set(self._h, None, 0, dim, self.index_base, 0), "fr_gallery_set")  # base, dim
        if rows is not None:
            self.add(rows)

    @property
    def ntotal(self) -> int:
        return self._n

    def reset(self) -> None:
        self._n = 0
        N.check(N.lib().fr_gallery_set(self._h, None, 0, self.d, self.index_base, 0), "fr_gallery_set")

    def _write(self, row0: int, rows) -> int:
        """fr_gallery_write of rows [row0, row0 + n) from host or device memory; returns n."""
        import torch

        r = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(np.asarray(rows, np.float32)))
        r = r.detach().float().reshape(-1, self.d).contiguous()
        n = int(r.shape[0])
        if n:
            N.check(N.lib().fr_gallery_write(self._h, N.ptr(r), int(row0), n, self.d, int(r.is_cuda)),
                    "fr_gallery_write")
        return n

    def add(self, rows) -> None:
        """Append rows (IndexFlatIP.add): written in place on the device, amortised O(new rows)."""
        self._n += self._write(self._n, rows)

    def update(self, row0: int, rows) -> None:
        """Overwrite rows [row0, row0 + n) (a dict-db entry re-embedded); row0 + n may run past the end."""
        if not 0 <= row0 <= self._n:
            raise IndexError(f"row {row0} outside a {self._n}-row gallery")
        self._n = max(self._n, row0 + self._write(row0, rows))

    def set_device_rows(self, rows_dev) -> None:
        """Install rows already resident on the GPU (no host round trip; the library copies them)."""
        rows_dev = rows_dev.float().contiguous()
        N.check(N.lib().fr_gallery_set(self._h, N.ptr(rows_dev), int(rows_dev.shape[0]), self.d, self.index_base, 1),
                "fr_gallery_set")
        self._n = int(rows_dev.shape[0])

    def set_exact(self, exact: bool) -> None:
        """FR_OPT_MATCH_EXACT: force the f32-MFMA kernel (default: bf16x3 candidates + exact rescoring
        for galleries of >= FR_OPT_X3_MIN_ROWS rows; both return the exact f32 top-k)."""
        N.check(N.lib().fr_set_option(self._h, N.FR_OPT_MATCH_EXACT, int(bool(exact))), "fr_set_option")

    def fallbacks(self) -> int:
        """Probes whose bf16x3 candidate proof failed and were rescanned exactly (device sync)."""
        return int(N.lib().fr_debug_match_fallbacks(self._h))

    def search_device(self, probes_dev, k: int, out_s=None, out_i=None):
        """probes_dev: cuda f32 [B, D] → (scores [B,k] f32, idx [B,k] int32) on the device, written into
        out_s / out_i when given (contiguous [B, k] f32 / int32 device tensors: no allocation)."""
        import torch

        p = probes_dev.float().contiguous()
        B = int(p.shape[0])
        s = out_s if out_s is not None else torch.empty((B, k), dtype=torch.float32, device=self.device)
        i = out_i if out_i is not None else torch.empty((B, k), dtype=torch.int32, device=self.device)
        if tuple(s.shape) != (B, k) or tuple(i.shape) != (B, k) or not (s.is_contiguous() and i.is_contiguous()) \
                or s.dtype != torch.float32 or i.dtype != torch.int32:
            raise ValueError(f"search_device: out_s / out_i must be contiguous [{B}, {k}] float32 / int32")
        N.check(N.lib().fr_match_topk(self._h, N.ptr(p), B, k, N.ptr(s), N.ptr(i), N.stream_ptr(self.device)),
                "fr_match_topk")
        return s, i

    def search(self, probes, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """IndexFlatIP.search: (scores [B,k] f32, ids [B,k] int64, -1 where fewer than k rows)."""
        import torch

        p = torch.as_tensor(np.asarray(probes, dtype=np.float32) if not torch.is_tensor(probes) else probes)
        p = p.reshape(-1, self.d).to(self.device)
        if p.shape[0] == 0:
            return np.zeros((0, k), np.float32), np.zeros((0, k), np.int64)
        if self.ntotal == 0:
            B = p.shape[0]
            return np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int64)
        s, i = self.search_device(p, k)
        return s.cpu().numpy(), i.cpu().numpy().astype(np.int64)

    def evaluate_device(self, probes_dev, true_idx_dev, k: int = 5, hist_bins: int = 0,
                        hist_range: Tuple[float, float] = (-1.0, 1.0), hist=None):
        """Labelled evaluation on the device (fr_match_eval): probes_dev cuda f32 [B, D], true_idx_dev cuda
        int32 [B] (each probe's true gallery row, a global index as ``search`` returns them).  Returns a
        dict of device tensors: ``scores`` / ``idx`` [B, k] exactly as ``search_device`` (None with k = 0),
        ``true_score`` [B] f32, ``true_rank`` [B] int32 (0-based position of the true row in the match
        order; -1 and -inf for a row outside this shard) and ``hist`` [hist_bins] int64, the counts of all
        impostor scores over ``hist_range`` (None with hist_bins = 0).  Pass the ``hist`` of an earlier
        call to accumulate over probe chunks."""
        import torch

        p = probes_dev.float().contiguous()
        B = int(p.shape[0])
        t = true_idx_dev.to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(t.shape) != (B,):
            raise ValueError(f"evaluate_device: true_idx must be [{B}]")
        s = torch.empty((B, k), dtype=torch.float32, device=self.device) if k else None
        i = torch.empty((B, k), dtype=torch.int32, device=self.device) if k else None
        ts = torch.empty((B,), dtype=torch.float32, device=self.device)
        tr = torch.empty((B,), dtype=torch.int32, device=self.device)
        if hist_bins and hist is None:
            hist = torch.zeros((hist_bins,), dtype=torch.int64, device=self.device)
        if hist is not None and (hist.dtype != torch.int64 or tuple(hist.shape) != (hist_bins,)
                                 or not hist.is_contiguous() or not hist.is_cuda):
            raise ValueError(f"evaluate_device: hist must be a contiguous cuda int64 [{hist_bins}]")
        N.check(N.lib().fr_match_eval(self._h, N.ptr(p), B, N.ptr(t), k, N.ptr(s), N.ptr(i), N.ptr(ts), N.ptr(tr),
                                      N.ptr(hist), hist_bins, float(hist_range[0]), float(hist_range[1]),
                                      N.stream_ptr(self.device)), "fr_match_eval")
        return {"scores": s, "idx": i, "true_score": ts, "true_rank": tr, "hist": hist}

    def evaluate(self, probes, true_idx, k: int = 5, hist_bins: int = 0,
                 hist_range: Tuple[float, float] = (-1.0, 1.0), chunk: int = 8192) -> dict:
        """``evaluate_device`` with numpy in and out (idx / true_rank / hist as int64).  Probes go to the
        device ``chunk`` rows at a time; the histogram accumulates over the chunks."""
        import torch

        p = torch.as_tensor(np.asarray(probes, dtype=np.float32) if not torch.is_tensor(probes) else probes)
        p = p.reshape(-1, self.d)
        t = torch.as_tensor(np.asarray(true_idx).astype(np.int32) if not torch.is_tensor(true_idx) else true_idx)
        t = t.reshape(-1)
        B = int(p.shape[0])
        if int(t.shape[0]) != B:
            raise ValueError("evaluate: one true_idx per probe")
        if self.ntotal == 0:
            raise RuntimeError("evaluate: empty gallery")
        parts = []
        hist = None
        for b0 in range(0, B, chunk):
            r = self.evaluate_device(p[b0:b0 + chunk].to(self.device), t[b0:b0 + chunk].to(self.device), k,
                                     hist_bins, hist_range, hist)
            hist = r["hist"]
            parts.append(r)

        if not parts:
            raise ValueError("evaluate: no probes")

        def cat(key, dtype):
            if parts[0][key] is None:
                return None
            return torch.cat([q[key] for q in parts]).cpu().numpy().astype(dtype)

        return {"scores": cat("scores", np.float32), "idx": cat("idx", np.int64),
                "true_score": cat("true_score", np.float32), "true_rank": cat("true_rank", np.int64),
                "hist": None if hist is None else hist.cpu().numpy()}

    def range_search_device(self, probes_dev, thresh: float, after=None):
        """Every gallery row scoring >= thresh per probe (fr_match_range_count / _fill): probes_dev cuda f32
        [B, D]; ``after`` None or int32 [B] of global indices (probe b keeps only rows with index >
        after[b]).  Returns device tensors ``(lims int64 [B + 1], scores f32 [T], idx int32 [T])``: probe b's
        hits are ``[lims[b], lims[b + 1])``, in ascending index.  Reading the total ``lims[-1]`` to size the
        output is the one synchronisation.  Note faiss's range_search is strict (>); this is >=, the
        reference's known-iff-not-below-threshold rule."""
        import torch

        p = probes_dev.float().contiguous()
        B = int(p.shape[0])
        if B == 0 or self.ntotal == 0:
            return (torch.zeros((B + 1,), dtype=torch.int64, device=self.device),
                    torch.empty((0,), dtype=torch.float32, device=self.device),
                    torch.empty((0,), dtype=torch.int32, device=self.device))
        a = None
        if after is not None:
            a = after.to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(a.shape) != (B,):
                raise ValueError(f"range_search_device: after must be [{B}]")
        L = N.lib()
        ws_bytes = int(L.fr_match_range_workspace(self._h, B))
        if ws_bytes <= 0:
            N.check(-1, "fr_match_range_workspace")
        ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.int32, device=self.device)
        lims = torch.empty((B + 1,), dtype=torch.int64, device=self.device)
        st = N.stream_ptr(self.device)
        N.check(L.fr_match_range_count(self._h, N.ptr(p), B, float(thresh), N.ptr(a), N.ptr(ws), N.ptr(lims), st),
                "fr_match_range_count")
        total = int(lims[-1].item())
        s = torch.empty((total,), dtype=torch.float32, device=self.device)
        i = torch.empty((total,), dtype=torch.int32, device=self.device)
        if total:
            N.check(L.fr_match_range_fill(self._h, N.ptr(p), B, float(thresh), N.ptr(a), N.ptr(ws), N.ptr(lims),
                                          N.ptr(s), N.ptr(i), total, st), "fr_match_range_fill")
        return lims, s, i

    def range_search(self, probes, thresh: float, order: str = "index", chunk: int = 8192,
                     max_hits: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """IndexFlatIP.range_search with >= instead of faiss's >: numpy ``(lims int64 [B + 1], D f32 [T],
        I int64 [T])``.  ``order="index"`` leaves each probe's hits in ascending index, ``"score"`` puts
        them in the match order (score descending, index ascending).  Probes go to the device ``chunk``
        rows at a time; RuntimeError once the total passes ``max_hits``."""
        import torch

        if order not in ("index", "score"):
            raise ValueError("range_search: order is 'index' or 'score'")
        p = torch.as_tensor(np.asarray(probes, dtype=np.float32) if not torch.is_tensor(probes) else probes)
        p = p.reshape(-1, self.d)
        B = int(p.shape[0])
        lims = np.zeros(B + 1, np.int64)
        if B == 0 or self.ntotal == 0:
            return lims, np.zeros(0, np.float32), np.zeros(0, np.int64)
        D_parts, I_parts, total = [], [], 0
        for b0 in range(0, B, chunk):
            l, s, i = self.range_search_device(p[b0:b0 + chunk].to(self.device), thresh)
            nb = int(l.shape[0]) - 1
            if order == "score" and int(s.shape[0]):
                seg = torch.repeat_interleave(torch.arange(nb, device=self.device), l[1:] - l[:-1])
                o1 = torch.sort(s, descending=True, stable=True)[1]  # ties keep ascending index
                o = o1[torch.sort(seg[o1], stable=True)[1]]
                s, i = s[o], i[o]
            lims[b0 + 1:b0 + nb + 1] = total + l[1:].cpu().numpy()
            total = int(lims[b0 + nb])
            if max_hits is not None and total > max_hits:
                raise RuntimeError(f"range_search: more than max_hits = {max_hits} hits")
            D_parts.append(s.cpu().numpy())
            I_parts.append(i.cpu().numpy().astype(np.int64))
        return lims, np.concatenate(D_parts), np.concatenate(I_parts)

    def reconstruct_n(self, row0: int = 0, n: Optional[int] = None, device: bool = False):
        """IndexFlatIP.reconstruct_n: the stored rows [row0, row0 + n) (local row numbers) as the match uses
        them, i.e. divided by their norm where it differed from 1 by >= 1e-3 (fr_gallery_read).  numpy
        [n, D] f32, or a device tensor with ``device=True``."""
        import torch

        n = self.ntotal - row0 if n is None else n
        if row0 < 0 or n < 0 or row0 + n > self.ntotal:
            raise IndexError(f"rows [{row0}, {row0 + n}) outside a {self.ntotal}-row gallery")
        out = torch.empty((n, self.d), dtype=torch.float32, device=self.device if device else "cpu")
        if n:
            N.check(N.lib().fr_gallery_read(self._h, int(row0), int(n), N.ptr(out), int(device)), "fr_gallery_read")
        return out if device else out.numpy()

    def self_pairs(self, thresh: float, chunk: int = 4096) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Every pair of gallery rows i < j with score >= thresh: numpy ``(i int64, j int64, score f32)`` in
        (i, j) ascending order, indices global.  The stored rows are read back on the device ``chunk`` at a
        time and searched as probes with ``after`` = their own index, so no N x N matrix exists anywhere
        (duplicate or mislabelled prototypes of a DatabaseBuilder gallery)."""
        import torch

        ii, jj, ss = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for r0 in range(0, self.ntotal, chunk):
            m = min(chunk, self.ntotal - r0)
            own = torch.arange(r0, r0 + m, device=self.device, dtype=torch.int64) + self.index_base
            l, s, j = self.range_search_device(self.reconstruct_n(r0, m, device=True), thresh, own.to(torch.int32))
            ii.append(torch.repeat_interleave(own, l[1:] - l[:-1]).cpu().numpy())
            jj.append(j.cpu().numpy().astype(np.int64))
            ss.append(s.cpu().numpy())
        return np.concatenate(ii), np.concatenate(jj), np.concatenate(ss)

    def close(self) -> None:
        if self._own and getattr(self, "_h", None):
            N.lib().fr_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
