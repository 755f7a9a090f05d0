"""MatteChain (voicepuppet_amd.matte_chain) against KeyMatte, MatteCleaner and MatteSolver called by hand in the dataset tool's order, each
with fresh outputs: byte for byte, over batches of 2 and 1 so that the second batch reuses the planes the first one wrote.  What the
stages compute is pinned by their own tests; this one pins the order, the arguments and the buffers.  The scene (48 x 80: ragged
32-pixel tiles, sides that differ) gives every stage work: stray components and a hole for the cleaner, an unknown band for the solve."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import matte_clean_ref as mr  # noqa: E402

N, H, W, BATCH = 3, 48, 80, 2
BATCHES = ((0, 2), (2, 3))
DESPILL = 0.5                                                     # the scene's backdrop is green by more than 16 levels: despill acts


@functools.lru_cache(maxsize=None)
def _inputs():
  import torch
  frames, _, _ = mr.scene(H, W, seed=11, n=N, spill_levels=10.0)
  return torch.from_numpy(frames).cuda(), torch.from_numpy(mr.landmarks(H, W, N)).cuda()


@functools.lru_cache(maxsize=None)
def _by_hand():
  """(alpha [3, H, W], foreground [3, H, W, 3], the key report, the clean report [3, 8], the solve report's fields): read-only"""
  from voicepuppet_amd.matte import KeyMatte
  from voicepuppet_amd.matte_clean import MatteCleaner
  from voicepuppet_amd.matte_solve import MatteSolver
  frames, anchors = _inputs()
  keyer = KeyMatte(N, H, W, max_radius=4).fit(frames)
  cleaner, solver = MatteCleaner(BATCH, H, W), MatteSolver(BATCH, H, W, max_radius=1)
  alphas, fores, clean_reports, solve_reports = [], [], [], []
  for lo, hi in BATCHES:
    a = keyer.matte(frames[lo:hi], lo=4.0, hi=10.0, radius=4, eps=25.0)
    a = cleaner.clean(a.contiguous(), anchors=anchors[lo:hi])
    clean_reports.append(cleaner.report())
    tri = solver.trimap(a.contiguous())
    a = solver.solve(frames[lo:hi], tri)
    solve_reports.append(solver.report())
    fores.append(keyer.foreground(frames[lo:hi], a.contiguous(), despill=DESPILL).cpu().numpy())
    alphas.append(a.cpu().numpy())
  res = (np.concatenate(alphas), np.concatenate(fores), keyer.report(), np.concatenate(clean_reports),
         {k: np.concatenate([r[k] for r in solve_reports]) for k in solve_reports[0]})
  for a in (res[0], res[1], res[3]) + tuple(res[4].values()):
    a.setflags(write=False)
  return res


def _full_chain():
  from voicepuppet_amd.matte_chain import MatteChain
  frames, _ = _inputs()
  chain = MatteChain(BATCH, H, W)
  chain.add_key(frames).add_clean().add_solve().add_foreground(despill=DESPILL)
  return chain


def test_chain_equals_the_stages_by_hand():
  from voicepuppet_amd import matte_clean, matte_solve
  frames, anchors = _inputs()
  want_alpha, want_fore, want_key, want_clean, want_solve = _by_hand()
  # the scene gives every stage work, so a skipped stage cannot pass: components to remove, a hole to fill, a band to solve
  assert (want_clean[:, 0] > want_clean[:, 1]).all() and (want_clean[:, 4] >= 1).all() and (want_clean[:, 6] == 0).all()
  assert (want_solve["unknown"] > 0).all() and (want_solve["iterations"] > 1).all() and (want_solve["status"] == 0).all()
  assert want_key["status"] == 0
  chain = _full_chain()
  try:
    assert chain.keyer.max_frames == N and chain.cleaner.max_frames == BATCH and chain.solver.max_radius == 1
    for lo, hi in BATCHES:
      fore, alpha = chain.run(frames[lo:hi], anchors=anchors[lo:hi])          # views that the next run overwrites: compared now
      assert tuple(alpha.shape) == (hi - lo, H, W) and tuple(fore.shape) == (hi - lo, H, W, 3)
      assert np.array_equal(alpha.cpu().numpy(), want_alpha[lo:hi]), (lo, hi)
      assert np.array_equal(fore.cpu().numpy(), want_fore[lo:hi]), (lo, hi)
    rep = chain.reports()
    assert sorted(rep) == ["clean", "key_matte", "solve"]
    assert rep["key_matte"] == want_key
    assert rep["clean"].dtype == np.int32 and np.array_equal(rep["clean"], want_clean)
    assert sorted(rep["solve"]) == sorted(want_solve)
    for k in want_solve:
      assert rep["solve"][k].dtype == want_solve[k].dtype and np.array_equal(rep["solve"][k], want_solve[k]), k
    text, warnings, fatal = chain.summary()
    assert text == ('; key matte: kept %.2f, residual %.1f levels' % (want_key['kept'], want_key['residual_rms'])
                    + '; clean: ' + matte_clean.summary(want_clean) + '; ' + matte_solve.summary(want_solve, 512, 1e-6)[0])
    assert warnings == [] and fatal is None
  finally:
    chain.close()


def test_model_only_chain_takes_the_matte_it_is_given():
  """The --alpha_dir --key_foreground path: the backdrop model without the key, foreground on a matte that is passed in."""
  import torch
  from voicepuppet_amd.matte import KeyMatte
  from voicepuppet_amd.matte_chain import MatteChain
  frames, _ = _inputs()
  given = torch.from_numpy(np.array(_by_hand()[0][:BATCH])).cuda()
  want = KeyMatte(N, H, W, max_radius=0).fit(frames).foreground(frames[:BATCH], given, despill=DESPILL).cpu().numpy()
  chain = MatteChain(BATCH, H, W).add_key(frames, matte=False).add_foreground(despill=DESPILL)
  try:
    assert chain.keyer.max_radius == 0
    fore, alpha = chain.run(frames[:BATCH], alpha=given)
    assert alpha is given
    assert np.array_equal(fore.cpu().numpy(), want)
    assert sorted(chain.reports()) == ["key_matte"]
    assert chain.summary() == ("", [], None)                      # the key's words belong to the key's matte
  finally:
    chain.close()


def test_close_twice_and_empty_chain():
  from voicepuppet_amd.matte_chain import MatteChain
  frames, _ = _inputs()
  chain = _full_chain()
  chain.close()
  assert chain.keyer.h is None and chain.cleaner.h is None and chain.solver.h is None
  chain.close()
  empty = MatteChain(BATCH, H, W)
  out, alpha = empty.run(frames[:1])
  assert alpha is None and out.data_ptr() == frames.data_ptr()
  assert empty.reports() == {} and empty.summary() == ("", [], None)
  empty.close()
