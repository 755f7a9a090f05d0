"""The matte stages as one sequence on the device: key -> clean -> solve -> foreground (KeyMatte.matte, MatteCleaner.clean,
MatteSolver.trimap and solve, KeyMatte.foreground).  A MatteChain owns the stages that were added, their reusable output planes and
their reports; run() is the one place that states the order.  It is what datasets/make_triptychs.py runs per batch, and the way to
run the same chain without that tool (an enrolment photo's matte, a clip's mattes for another writer).

  chain = MatteChain(max_frames, height, width)
  chain.add_key(fit_frames)          # each add_* is optional and builds its stage at once: a refusal is that stage's own exception
  chain.add_clean()
  chain.add_solve()
  chain.add_foreground()
  for each batch: frames_out, alpha = chain.run(frames, anchors=landmark_pixels)
  chain.summary(), chain.reports(), chain.close()

It neither logs nor exits, parses no options and reads no files; write_alpha writes PNGs.
"""
import numpy as np
import torch

from . import matte_clean, matte_solve
from .matte import STATUS_TEXT, KeyMatte


class MatteChain:
  """Stages for batches of at most max_frames device uint8 RGB frames [n, height, width, 3]."""

  def __init__(self, max_frames, height, width):
    self.max_frames, self.height, self.width = int(max_frames), int(height), int(width)
    self.keyer = self.cleaner = self.solver = None
    self._key = self._clean = self._solve = self._despill = None           # a stage's run-time parameters; None: no such stage
    self._key_report, self._clean_reports, self._solve_reports = None, [], []

  def _plane(self):
    return torch.empty(self.max_frames, self.height, self.width, dtype=torch.uint8, device="cuda")

  def add_key(self, fit_frames, matte=True, lo=4.0, hi=10.0, radius=4, eps=25.0, band=None):
    """The backdrop model, fitted here to the border of fit_frames [k, height, width, 3] (one host read: its report).  matte=True: run
    computes the matte with KeyMatte.matte(lo, hi, radius, eps); matte=False: the model alone, for add_foreground on a matte that is
    passed to run (no guided-filter planes in the workspace)."""
    self.keyer = KeyMatte(max(self.max_frames, int(fit_frames.shape[0])), self.height, self.width, max_radius=radius if matte else 0)
    self.keyer.fit(fit_frames, band=band)
    self._key_report = self.keyer.report()
    self._key = dict(lo=lo, hi=hi, radius=radius, eps=eps) if matte else None
    return self

  def add_clean(self, support=32, core=224, min_area=None, max_hole=None, grow=4, keep="anchored"):
    """MatteCleaner.clean with these parameters on the matte so far; run's anchors go to it."""
    self.cleaner = matte_clean.MatteCleaner(self.max_frames, self.height, self.width)
    self._cleaned = self._plane()
    self._clean = dict(support=support, core=core, min_area=min_area, max_hole=max_hole, grow=grow, keep=keep)
    return self

  def add_solve(self, erode=None, dilate=None, radius=1, eps=matte_solve.DEFAULT_EPS, iters=matte_solve.DEFAULT_ITERS, tol=matte_solve.DEFAULT_TOL):
    """MatteSolver.trimap(erode, dilate) of the matte so far, then MatteSolver.solve(radius, eps, iters, tol) on the frames."""
    self.solver = matte_solve.MatteSolver(self.max_frames, self.height, self.width, max_radius=radius)
    self._trimap, self._solved = self._plane(), self._plane()
    self._trimap_args, self._solve = dict(erode=erode, dilate=dilate), dict(radius=radius, eps=eps, iters=iters, tol=tol)
    return self

  def add_foreground(self, despill=0.0):
    """The frames run returns become KeyMatte.foreground(frames, matte, despill): needs add_key, with matte=False for a matte from files."""
    if self.keyer is None:
      raise ValueError("add_foreground: the backdrop model of add_key is needed")
    self._despill = despill
    return self

  def run(self, frames, alpha=None, anchors=None):
    """One batch through the stages that exist -> (frames, alpha).  frames: device uint8 [n, height, width, 3], n <= max_frames; alpha:
    the matte [n, height, width] to start from when no key stage computes it; anchors: int32 [n, k, 2] for the clean stage.  Only
    enqueues on the current stream, but for the host read of the clean and the solve report of the batch.  What it returns are views
    of the chain's own planes (or the arguments, with no stage): they live until the next run."""
    if self._key is not None:
      alpha = self.keyer.matte(frames, **self._key)
    if self.cleaner is not None:
      alpha = self.cleaner.clean(alpha.contiguous(), anchors=anchors, out=self._cleaned, **self._clean)
      self._clean_reports.append(self.cleaner.report())
    if self.solver is not None:
      tri = self.solver.trimap(alpha.contiguous(), out=self._trimap, **self._trimap_args)
      alpha = self.solver.solve(frames, tri, out=self._solved, **self._solve)
      self._solve_reports.append(self.solver.report())
    if self._despill is not None:
      frames = self.keyer.foreground(frames, alpha.contiguous(), despill=self._despill)
    return frames, alpha

  def write_alpha(self, alpha, dir, first_index):
    """alpha [n, height, width] -> <first_index + i>.png in `dir` (KeyMatte.write_png); returns the paths."""
    if self.keyer is None:
      raise ValueError("write_alpha: the chain has no key stage")
    return self.keyer.write_png(alpha, dir, first_index)

  def reports(self):
    """Of the stages that exist, over all runs so far: {'key_matte': KeyMatte.report() of the fit, 'clean': int32 [frames, 8],
    'solve': {field: array [frames]}}."""
    res = {}
    if self._key_report is not None:
      res["key_matte"] = self._key_report
    if self.cleaner is not None:
      res["clean"] = np.concatenate(self._clean_reports)
    if self.solver is not None:
      res["solve"] = {k: np.concatenate([r[k] for r in self._solve_reports]) for k in self._solve_reports[0]}
    return res

  def summary(self):
    """-> (the stages' part of the dataset tool's line, [warnings], a fatal finding or None) over all runs so far.  After a fatal
    finding nothing more is added."""
    rep, text, warnings = self.reports(), "", []
    if self._key is not None:
      key = rep["key_matte"]
      text += '; key matte: kept %.2f, residual %.1f levels' % (key['kept'], key['residual_rms'])
      if key['status'] != 0:
        warnings.append('key matte status %d: %s' % (key['status'], STATUS_TEXT.get(key['status'], '?')))
      if key['kept'] < 0.5:
        warnings.append('key matte: the robust pass kept %.2f of the border samples: the border is not a plain backdrop' % key['kept'])
    if self.cleaner is not None:
      text += '; clean: ' + matte_clean.summary(rep["clean"])
      if (rep["clean"][:, 6] & 1).any():
        warnings.append('matte clean: no component of %d frames held a landmark or reached the bottom edge; they were left as they were'
                        % int((rep["clean"][:, 6] & 1).sum()))
      if (rep["clean"][:, 6] & 2).any():
        return text, warnings, 'matte clean: the labelling reached a step cap (a bug); the mattes are not to be used'
    if self.solver is not None:
      solve_text, flagged, capped = matte_solve.summary(rep["solve"], self._solve["iters"], self._solve["tol"])
      text += '; ' + solve_text
      if flagged:
        warnings.append('matte solve: %d frames ended with a status bit set (1: nothing to solve or no constraint reaches the band; 2: the '
                        'iteration broke down)' % flagged)
      if capped:
        warnings.append('matte solve: %d frames ran all %d iterations without reaching the residual %g'
                        % (capped, self._solve["iters"], self._solve["tol"]))
    return text, warnings, None

  def close(self):
    """Destroys the stages' handles now; a second call does nothing."""
    for stage in (self.keyer, self.cleaner, self.solver):
      if stage is not None:
        stage.close()
