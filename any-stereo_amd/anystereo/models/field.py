"""A finished pass as a continuous field.  After the GRU loop the disparity at any coordinate is one upsampler pass over
(disp, hidden state, stem_4x, stem_2x): `model.encode(...)` runs the pre-loop and the loop once and returns a `StereoField`;
`field.query(hr_coord, scale)` is `upsample_disp` on the kept state — a second query set on the same pair (another scale, a region of
interest, a zoom) or the prediction of an earlier GRU iteration costs that pass, not a forward.

    field = model.encode(image1, image2, iters=32, at=(4, 8, 16, 32))
    up = field.query(hr_coord, scale)                 # [B,1,Q], what forward(..., iters=32) returns
    curve = field.query(hr_coord, scale, at="all")    # [4,B,1,Q]
    low = field.low(at=8)                             # [B,1,h,w]
"""
from __future__ import annotations

import operator

import torch

from .. import ops


def normalize_at(at, iters: int):
    """`at` of encode -> ascending tuple of distinct 1-based iterations in [1, iters] that ends with `iters`."""
    if at is None:
        return (iters,)
    try:
        ks = [int(k) for k in at]
        exact = all(float(k) == int(k) for k in at)
    except (TypeError, ValueError):
        raise ValueError(f"encode: at must be an iterable of 1-based iterations, got {at!r}") from None
    if not exact or any(k < 1 or k > iters for k in ks):
        raise ValueError(f"encode: at = {tuple(at)!r} has an entry outside [1, {iters}] (1-based GRU iterations)")
    return tuple(sorted(set(ks) | {iters}))


class StereoField:
    """What `encode` kept: per kept iteration k the 1/4-resolution disparity and the first hidden state after k GRU iterations, per
    field the stems the upsampler reads, the model's weights fingerprint and the precision mode.

    Rows of the upsampler's inputs (affinity + first MLP layer at low resolution, the fused tail's operands) are cached where the
    fused tail runs: those of stem_2x once per field — they serve every later query and every `at` — and those of
    (stem_4x, hidden state) once per kept iteration.  The staged / general upsampler paths recompute per query."""

    def __init__(self, model, iters, at, state, fingerprint, mode):
        self._model = model
        self.iters = int(iters)
        self.at = tuple(at)
        self._disp = dict(zip(self.at, state["disp"]))
        self._net = dict(zip(self.at, state["net"]))
        self._stem_4x, self._stem_2x, self._stem_1x = state["stems"]
        self._fingerprint = fingerprint
        self._mode = mode
        self._rows_static = None  # the loop-invariant input's rows (slot 1 of the fused tail)
        self._rows = {}           # kept iteration -> the hidden-state input's rows (slot 0)

    def _pick(self, at):
        if at is None:
            return self.at[-1]
        try:
            k = operator.index(at)
        except TypeError:
            k = None
        if k not in self._disp:
            raise ValueError(f"StereoField: iteration {at!r} was not kept (kept: {self.at})")
        return k

    def _check(self):
        m = self._model
        if m._weights_fingerprint() != self._fingerprint:
            raise RuntimeError("StereoField.query: the model's weights changed since encode() (optimizer step, load_state_dict, .to()): "
                               "the kept state belongs to the old weights — encode again")
        if ops.get_precision() != self._mode[0]:
            raise RuntimeError(f"StereoField.query: set_precision changed the mode from {self._mode[0]!r} to {ops.get_precision()!r} "
                               "since encode() — encode again")
        if m.training:
            raise RuntimeError("StereoField.query: the model is in training mode")

    def low(self, at=None) -> torch.Tensor:
        """[B,1,h,w]: a clone of the 1/4-resolution disparity after iteration `at` (default: the last kept one)."""
        return self._disp[self._pick(at)].clone()

    @torch.no_grad()
    def query(self, hr_coord, scale, at=None) -> torch.Tensor:
        """hr_coord [B,Q,2] (row, col in [-1,1]), scale as in forward -> [B,1,Q] for iteration `at` (None: the last kept one), or
        [m,B,1,Q] over all kept iterations for at="all".  Runs the path `upsample_disp` runs in forward: the fused tail where it
        applies, the staged or general path otherwise; any Q, raster or unordered coordinates, any number of calls.
        As forward does, it clamps the caller's `hr_coord` IN PLACE to [-1 + 1e-6, 1 - 1e-6] (the reference's side effect,
        submodule.py:366): pass a clone to keep the coordinates."""
        self._check()
        ks = self.at if (isinstance(at, str) and at == "all") else (self._pick(at),)
        m = self._model
        if self._mode[1] and not ops.get_fast_fp16():
            with ops.fast_fp16(True):
                return self.query(hr_coord, scale, at)
        outs = []
        for i, k in enumerate(ks):
            # every iteration sees the coordinates as given: the path reads them before it clamps them, so only the last call gets
            # the caller's tensor (and leaves it clamped)
            coord = hr_coord if i + 1 == len(ks) else hr_coord.clone()
            outs.append(self._upsample(m, k, coord, scale))
        return outs[0] if not (isinstance(at, str) and at == "all") else torch.stack(outs, 0)

    def _upsample(self, m, k, coord, scale):
        liif = getattr(m, "liif_up", None)
        cache = {}
        if self._rows_static is not None:
            cache[1] = self._rows_static
        if k in self._rows:
            cache[0] = self._rows[k]
        if liif is not None:
            liif.__dict__["_field_rows"] = cache
        try:
            up = m.upsample_disp(self._disp[k], self._net[k], self._stem_4x, self._stem_2x, self._stem_1x, hr_coord=coord, scale=scale)
        finally:
            if liif is not None:
                liif.__dict__.pop("_field_rows", None)
        if 1 in cache:
            self._rows_static = cache[1]
        if 0 in cache:
            self._rows[k] = cache[0]
        return up
