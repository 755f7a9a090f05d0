"""Frames for stream groups on the device (voicepuppet_amd.stream.PuppetStreamGroup, libvp_hip.so vp_puppet_* / vp_bfm_reconstruct_rows):
each new kernel against the expressions it replaces, bit for bit, and the group against one-slot streams fed the same chunks.  Assets are
the synthetic ones of tests/test_gpu_stream_cli.py (synthetic face model, random but saved checkpoints), one photo and coefficient file
per talker."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "params.yml")
H = 512

# (ratio, transform_params, center_x, center_y): face sides 224 (copy), 112 (exact 2x reduction), 187 and 320 (bilinear, below and above
# 224); the 320 one hangs over the canvas's right and bottom edges, the 112 one is shifted by its transform parameters
GEOMETRY = [(1.0, [512, 512, 1.0, 0.0, 0.0], 256, 256),
            (2.0, [512, 512, 1.0, 30.0, -50.0], 200, 300),
            (1.2, [512, 512, 1.0, 0.0, 0.0], 100, 90),
            (0.7, [512, 512, 1.0, 0.0, 0.0], 400, 430)]


def _bits(t):
  import torch
  return t.contiguous().view(torch.int32)


def _facemodel_mat():
  from scipy.io import savemat
  from oracle import bfm_ref as br
  fm = br.synthetic_facemodel(3)
  os.makedirs("BFM")
  savemat(os.path.join("BFM", "BFM_model_front.mat"),
          {"meanshape": fm.meanshape, "idBase": fm.idBase, "exBase": fm.exBase, "meantex": fm.meantex, "texBase": fm.texBase,
           "point_buf": fm.point_buf, "tri": fm.tri, "keypoints": (fm.keypoints + 1).reshape(1, -1)})


def _photo_npz(i, path):
  from oracle import bfm_ref as br
  ratio, tp, cx, cy = GEOMETRY[i]
  coeff, _ = br.synthetic_coeffs(1, 5 + i)
  np.savez(path, bfmcoeff=coeff.reshape(1, 257), transform_params=np.array(tp, np.float32), center_x=cx, center_y=cy, ratio=ratio)


def _backgrounds(which=(1, 2, 5)):
  from PIL import Image
  os.makedirs("background")
  rng = np.random.default_rng(1)
  for i in which:
    Image.fromarray((rng.uniform(size=(H, H, 3)) * 255).astype(np.uint8)).save(os.path.join("background", "%d.jpg" % i))


def _assets(talkers, samples):
  """face<i>.jpg, a<i>.wav, photo<i>.npz per talker, the face model, both checkpoints, three backgrounds (tests/test_gpu_stream_cli.py's
  recipe)."""
  from PIL import Image
  from scipy.io import wavfile
  from voicepuppet_amd.bfmnet.bfmnet import random_variables
  from voicepuppet_amd.pixrefer import infer_bfmvid
  for i in range(talkers):
    rng = np.random.default_rng(10 + i)
    Image.fromarray((rng.uniform(size=(H, 3 * H, 3)) * 255).astype(np.uint8)).save("face%d.jpg" % i)
    t = np.arange(samples[i]) / 16000.0
    wavfile.write("a%d.wav" % i, 16000, (0.3 * np.sin(2 * np.pi * (330 + 110 * i) * t) * np.sin(2 * np.pi * (3 + i) * t) * 32767).astype(np.int16))
    _photo_npz(i, "photo%d.npz" % i)
  _facemodel_mat()
  os.makedirs("ckpt_bfmnet")
  np.savez(infer_bfmvid.BFMNET_CKPT + ".npz", **random_variables(seed=11))
  gen = infer_bfmvid.load_generator(CFG, 4, H)[0]
  os.makedirs("ckpt_pixrefer")
  np.savez(infer_bfmvid.PIX_CKPT + ".npz", **gen.engine.get_params(0))
  _backgrounds()


def _handle(slots, frame_batch):
  import torch
  from voicepuppet_amd import _lib
  from voicepuppet_amd.stream import puppet_desc
  L = _lib.lib()
  d = puppet_desc(slots, frame_batch, H)
  ws = L.vp_puppet_workspace_bytes(ctypes.byref(d))
  assert ws > 0
  w = torch.empty(ws, dtype=torch.uint8, device="cuda")
  h = ctypes.c_void_p()
  _lib.check(L.vp_puppet_create(ctypes.byref(d), ctypes.c_void_p(w.data_ptr()), ws, None, ctypes.byref(h)), "vp_puppet_create")
  return L, h, w


def _p(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_splice_equals_splice_coeff():
  """5 rows over 3 slots in permuted order: vp_puppet_splice gives infer_bfmvid.splice_coeff's rows bit for bit."""
  import torch
  from voicepuppet_amd import _lib
  from voicepuppet_amd.pixrefer.infer_bfmvid import splice_coeff
  L, h, w = _handle(3, 4)
  rng = np.random.default_rng(0)
  photo = rng.normal(size=(3, 257)).astype(np.float32)
  panel = torch.zeros(H, H, 3, device="cuda")
  for s in range(3):
    _lib.check(L.vp_puppet_attach(h, s, _p(panel), _p(panel), photo[s].ctypes.data_as(ctypes.c_void_p), 224, 0, 0, None), "attach")
  expr = rng.normal(size=(5, 64)).astype(np.float32)
  rows = np.array([[2, 4, 0, 0], [0, 0, 0, 0], [1, 3, 0, 0], [2, 1, 0, 0], [0, 2, 0, 0]], np.int32)
  out = torch.full((5, 257), float("nan"), device="cuda")
  expr_d, rows_d = torch.from_numpy(expr).cuda(), torch.from_numpy(rows).cuda()
  _lib.check(L.vp_puppet_splice(h, _p(expr_d), 5, _p(rows_d), 5, _p(out), None), "splice")
  want = np.stack([splice_coeff(photo[s].reshape(1, 257), expr[k].reshape(1, 1, 64))[0, 0] for s, k in rows[:, :2]])
  assert want.dtype == np.float32
  assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
  L.vp_puppet_destroy(h)


def test_mixed_identity_reconstruct_equals_one_call_per_identity():
  """Rows of 3 identities in one vp_bfm_reconstruct_rows call equal three vp_bfm_reconstruct(shared_texture=1) calls bit for bit in
  vertices and colors, and the rasterised images and masks are equal."""
  import torch
  from oracle import bfm_ref as br
  from voicepuppet_amd.utils.reconstruct_mesh import ClipRenderer, Compute_rotation_matrix, reconstruct_clip
  r = ClipRenderer(br.synthetic_facemodel(3))
  frames = (4, 1, 3)
  clips = [br.synthetic_coeffs(n, 20 + i) for i, n in enumerate(frames)]
  order = [(0, 0), (2, 0), (0, 1), (1, 0), (2, 1), (0, 2), (2, 2), (0, 3)]            # (identity, its frame), interleaved
  coeff = np.stack([clips[i][0][f] for i, f in order]).astype(np.float32)
  angles = np.stack([clips[i][1][f] for i, f in order]).astype(np.float32)
  ident = np.array([i for i, _ in order])
  present, first = np.unique(ident, return_index=True)
  tex_src = torch.from_numpy(first.astype(np.int32)).cuda()
  tex_row = torch.from_numpy(np.searchsorted(present, ident).astype(np.int32)).cuda()
  rot = torch.from_numpy(Compute_rotation_matrix(angles)).cuda()
  from voicepuppet_amd.utils.reconstruct_mesh import reconstruct_rows
  v, c = reconstruct_rows(torch.from_numpy(coeff).cuda(), rot, tex_src, 3, tex_row, r.model)
  img, mask = r.render_rows(torch.from_numpy(coeff).cuda(), rot, tex_src, 3, tex_row)
  v, c, img, mask = v.cpu().numpy(), c.cpu().numpy(), img.cpu().numpy(), mask.cpu().numpy()
  for i in range(3):
    rows = np.flatnonzero(ident == i)
    o = reconstruct_clip(coeff[rows], r.model, angles[rows], shared_texture=True, full=False)
    assert np.array_equal(o["vertices"].cpu().numpy().view(np.int32), v[rows].view(np.int32)), i
    assert np.array_equal(o["colors"].cpu().numpy().view(np.int32), c[rows].view(np.int32)), i
    wi, wm = r(coeff[rows], angles[rows])
    assert np.array_equal(wi.cpu().numpy(), img[rows]) and np.array_equal(wm.cpu().numpy(), mask[rows]), i
  assert img.any() and not np.array_equal(c[0], c[1])                                 # faces are drawn; identities do differ


def test_condition_kernel_equals_the_stream_expressions(tmp_path, monkeypatch):
  """vp_puppet_condition against what PuppetStream._frames wrote before stream groups: render_faces(on_device=True) ->
  .flip(-1).to(float32) / 255.0 for channels 3:6, the reference panels, background_target or 0.5.  Five slots: sides 224 (copy), 112 (2x
  reduction, shifted by transform parameters), 187 and 320 (bilinear; the 320 one hangs over two canvas edges), one without coefficients;
  backgrounds for some frame indices only.  Integer work followed by one float division: equality in float32 bits, no tolerance."""
  import torch
  from oracle import bfm_ref as br
  from voicepuppet_amd import _lib
  from voicepuppet_amd.pixrefer import infer_bfmvid as ib
  from voicepuppet_amd.stream import background_bank
  from voicepuppet_amd.utils.reconstruct_mesh import ClipRenderer
  monkeypatch.chdir(tmp_path)
  _backgrounds()
  nb = 8
  L, h, w = _handle(5, nb)
  r = ClipRenderer(br.synthetic_facemodel(3))
  rng = np.random.default_rng(3)
  refer = torch.from_numpy(rng.uniform(size=(5, H, H, 3)).astype(np.float32)).cuda()
  fg = torch.from_numpy(rng.uniform(size=(5, H, H, 3)).astype(np.float32)).cuda()
  kinds = []
  for s in range(5):
    if s < 4:
      _photo_npz(s, "p%d.npz" % s)
      p = np.load("p%d.npz" % s)
      side, y0, x0 = ib.paste_geometry(int(p["center_x"]), int(p["center_y"]), float(p["ratio"]), p["transform_params"], 224)
      coeff = np.ascontiguousarray(p["bfmcoeff"].reshape(257), np.float32)
      _lib.check(L.vp_puppet_attach(h, s, _p(refer[s]), _p(fg[s]), coeff.ctypes.data_as(ctypes.c_void_p), side, y0, x0, None), "attach")
    else:
      _lib.check(L.vp_puppet_attach(h, s, _p(refer[s]), _p(fg[s]), None, 0, 0, 0, None), "attach")
    info = (ctypes.c_int * 4)()
    _lib.check(L.vp_puppet_slot_info(h, s, info), "slot_info")
    kinds.append(tuple(info))
  assert [k[0] for k in kinds] == [2, 3, 4, 4, 1] and [k[1] for k in kinds[:4]] == [224, 112, 187, 320], kinds   # resize.hip modes 1, 2, 0, 0
  assert kinds[3][2] + 320 > H and kinds[3][3] + 320 > H                                # hangs over the bottom and right edges
  bank, bg_row = background_bank(H)
  assert bank.shape[0] == 3 and sorted(np.flatnonzero(bg_row >= 0)) == [0, 1, 4]
  _lib.check(L.vp_puppet_set_backgrounds(h, _p(bank), 3), "set_backgrounds")
  # 8 rows: (slot, global frame index); two frames for some slots
  rows = [(3, 0), (0, 1), (4, 4), (1, 7), (2, 100), (3, 101), (0, 2), (4, 55)]
  exprs = {s: br.synthetic_coeffs(4, 40 + s) for s in range(4)}
  faces, cond, want_face = [], [], {}
  for s in range(4):
    mine = [b for b, (ss, _) in enumerate(rows) if ss == s]
    p = np.load("p%d.npz" % s)
    seq = ib.splice_coeff(p["bfmcoeff"].reshape(1, 257), exprs[s][0][np.newaxis, :len(mine), 80:144])[0].astype(np.float32)
    ang = ib.angle_sequence(len(mine))
    canvas = ib.render_faces(r, int(p["center_x"]), int(p["center_y"]), float(p["ratio"]), seq, (H, H, 3), p["transform_params"],
                             on_device=True, angles=ang)
    f32 = canvas.flip(-1).to(torch.float32) / 255.0                                    # the expression of PuppetStream._frames
    imgs, _ = r(seq, ang)
    for j, b in enumerate(mine):
      want_face[b] = f32[j]
      cond.append((b, len(faces)))
      faces.append(imgs[j])
  faces = torch.stack(faces)
  assert faces.any()
  face_of = dict(cond)
  table = np.array([[s, face_of.get(b, -1), bg_row[g % 100], g] for b, (s, g) in enumerate(rows)], np.int32)
  inputs = torch.full((nb, H, H, 6), float("nan"), device="cuda")
  fgi = torch.full((nb, H, H, 3), float("nan"), device="cuda")
  tg = torch.full((nb, H, H, 3), float("nan"), device="cuda")
  table_d = torch.from_numpy(table).cuda()
  _lib.check(L.vp_puppet_condition(h, _p(faces), faces.shape[0], _p(table_d), nb, _p(inputs), _p(fgi), _p(tg), None),
             "vp_puppet_condition")
  torch.cuda.synchronize()
  for b, (s, g) in enumerate(rows):
    assert torch.equal(_bits(inputs[b, ..., 0:3]), _bits(refer[s])), b
    want = want_face[b] if s < 4 else refer[s]
    assert torch.equal(_bits(inputs[b, ..., 3:6]), _bits(want)), (b, s, float((inputs[b, ..., 3:6] - want).abs().max()))
    assert torch.equal(_bits(fgi[b]), _bits(fg[s])), b
    bgt = ib.background_target(g, H)
    want_t = torch.as_tensor(bgt).cuda() if bgt is not None else torch.full((H, H, 3), 0.5, device="cuda")
    assert (bgt is not None) == (g % 100 in (0, 1, 4))
    assert torch.equal(_bits(tg[b]), _bits(want_t)), (b, g)
  assert all(float(want_face[b].max()) > 0 for b in want_face)                          # every pasted face is on the canvas
  L.vp_puppet_destroy(h)


# ---- the group against one-slot streams ----------------------------------------------------------------------------------------------

FRAMES = (13, 30, 51, 51)
SAMPLES = tuple(640 * (f - 1) for f in FRAMES)


def _parity_rule():
  """profiles/puppet_group_parity.json: what moving one conditioned frame between batch rows and plans changes on the commit before
  stream groups for frames (max |d| of float Outputs and of uint8 frames)."""
  with open(os.path.join(ROOT, "profiles", "puppet_group_parity.json")) as f:
    p = json.loads(f.readline())
  return float(p["outputs_max_abs"]), int(p["u8_max_abs"])


def _compare_generated(got_f, want_f, got_u8, want_u8, what):
  """The rule of the issue: uint8 equality if the parent commit's own batch-row sensitivity is zero, else rel-L2 < 1e-5 on float
  Outputs and uint8 max |d| no larger than the parent's recorded value."""
  fmax, umax = _parity_rule()
  d8 = int(np.abs(got_u8.astype(np.int32) - want_u8.astype(np.int32)).max()) if got_u8.size else 0
  rel = None
  if got_f is not None:
    rel = float(np.linalg.norm((got_f - want_f).ravel()) / max(np.linalg.norm(want_f.ravel()), 1e-30))
  print("%s: uint8 max |d| %d (parent %d), Outputs rel-L2 %s (parent max |d| %.3g)" % (what, d8, umax, rel, fmax))
  if fmax == 0 and umax == 0:
    assert d8 == 0, what
  else:
    assert rel is None or rel < 1e-5, (what, rel)
    assert d8 <= umax, (what, d8, umax)


def _chunks(pcm, n):
  return [pcm[a:a + n] for a in range(0, len(pcm), n)]


def _schedule():
  """Per step {slot: chunk}, the slots finishing after that step's chunk, and the slots reset before it.  Slot 0: 40 ms chunks; slot 1:
  130 ms; slot 2: its whole clip in one push; slot 3 (no coefficients): 130 ms, reset after 9 pushes and run again from the start."""
  from voicepuppet_amd.generator.loader import WavLoader
  pcm = [WavLoader(sr=16000).get_data("a%d.wav" % i).astype(np.float32) for i in range(4)]
  per = [_chunks(pcm[0], 640), _chunks(pcm[1], 2080), [pcm[2]], _chunks(pcm[3], 2080)]
  lists = []
  for s in range(4):
    ev = [("push", c, i == len(per[s]) - 1) for i, c in enumerate(per[s])]
    if s == 3:
      ev = ev[:9] + [("reset", None, False)] + ev
      ev[8] = ("push", ev[8][1], False)
    if s == 2:
      ev = [("idle", None, False)] * 5 + ev                                             # the whole clip arrives in the sixth push
    lists.append(ev)
  steps = []
  for i in range(max(len(e) for e in lists)):
    chunk, fin, reset = {}, [], []
    for s in range(4):
      if i < len(lists[s]):
        kind, c, last = lists[s][i]
        if kind == "push":
          chunk[s] = c
          if last:
            fin.append(s)
        elif kind == "reset":
          reset.append(s)
    steps.append((chunk, fin, reset))
  return steps


NPZ = ["photo0.npz", "photo1.npz", "photo2.npz", None]


def _photos():
  from voicepuppet_amd.generator.loader import ImageLoader
  return [ImageLoader().get_data("face%d.jpg" % i)[:, :, ::-1] for i in range(4)]


def _group():
  from voicepuppet_amd.stream import PuppetStreamGroup
  g = PuppetStreamGroup(CFG, 4, frame_batch=4)
  for s, img in enumerate(_photos()):
    g.attach(s, img, NPZ[s])
  return g


def _group_and_singles():
  from voicepuppet_amd.stream import PuppetStream
  return _group(), [PuppetStream(CFG, img, bfmcoeff=NPZ[s], frame_batch=4) for s, img in enumerate(_photos())]


def _ears(group, chunk, fin, rng):
  k = group.audio.ready({s: len(c) for s, c in chunk.items()}, fin)
  return {s: rng.uniform(size=(k[s], 1)).astype(np.float32) / 100 for s in range(4) if k[s]}


def test_group_equals_talkers_alone(tmp_path, monkeypatch):
  """4 slots (three photos with their coefficient files, one without), clips of 13, 30, 51 and 51 frames, 40 ms / 130 ms / whole-clip
  chunking, one slot reset and run again mid-way, frame_batch 4, against a one-slot PuppetStream per talker fed the same chunks under
  the same ears: the same frame counts and global indices, conditioning tensors bit-identical row for row, generated frames under the
  parent commit's own batch-row sensitivity (profiles/puppet_group_parity.json)."""
  import torch
  monkeypatch.chdir(tmp_path)
  _assets(4, SAMPLES)
  g, singles = _group_and_singles()
  g.keep_conditioning = True
  for ps in singles:
    ps.group.keep_conditioning = True
  rng = np.random.default_rng(5)
  emitted = {s: [] for s in range(4)}
  worst = 0
  for chunk, fin, reset in _schedule():
    for s in reset:
      g.reset_slot(s)
      singles[s].reset()
      emitted[s] = []
    if not chunk and not fin:
      continue
    ears = _ears(g, chunk, fin, rng)
    res = g.push(chunk, finish=fin, ears=ears)
    cond = g.last_conditioning
    frames = g.last_frames.cpu().numpy() if g.last_frames is not None else None
    row = 0
    for s in sorted(res):
      one = singles[s].group.push({0: chunk[s]} if s in chunk else {}, finish=(0,) if s in fin else (), ears={0: ears[s]} if s in ears else None)
      assert [i for i, _ in res[s]] == [i for i, _ in one[0]], s                      # same frame counts and global indices
      emitted[s].extend(i for i, _ in res[s])
      k = len(res[s])
      if k == 0:
        continue
      rows = np.flatnonzero(cond["slot"] == s)
      assert len(rows) == k and cond["frame"][rows].tolist() == [i for i, _ in res[s]]
      oc = singles[s].group.last_conditioning
      for name in ("inputs", "fg_inputs", "targets"):
        assert torch.equal(_bits(cond[name][rows]), _bits(oc[name])), (s, name)
      want_u8 = singles[s].group.last_frames.cpu().numpy()
      _compare_generated(cond["Outputs"][rows].cpu().numpy(), oc["Outputs"].cpu().numpy(), frames[rows], want_u8, "slot %d frames %s" % (s, res[s][0][0]))
      worst = max(worst, int(np.abs(frames[rows].astype(np.int32) - want_u8.astype(np.int32)).max()))
      row += k
  assert [emitted[s] for s in range(4)] == [list(range(f)) for f in FRAMES]
  print("worst uint8 max |d| over the run: %d" % worst)


def _spin_cycles(ms):
  """torch.cuda._sleep cycles for about `ms` milliseconds, calibrated with events on this device."""
  import torch
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  torch.cuda._sleep(20_000_000)
  e1.record()
  e1.synchronize()
  per_ms = 20_000_000 / max(e0.elapsed_time(e1), 1e-3)
  return int(per_ms * ms)


def test_push_only_enqueues(tmp_path, monkeypatch):
  """No synchronising call inside push: with a spinning kernel on the stream ahead of it, push returns while an event recorded before
  the push is still pending.  The spin is 400 ms: profiles/puppet_group_latency.json puts the enqueue time of a 4-slot push at about one
  millisecond (enqueue_ms_median of the S = 4 rows: 0.9 - 1.2 ms), so 400 ms is some hundred times that, and a push that waited for the device
  anywhere would return only after the spin.  If the host is so slow that the event has completed, the test fails: it never passes
  without having seen the push return first.  Afterwards the frames are those of an identical group that ran without the spin."""
  import torch
  monkeypatch.chdir(tmp_path)
  _assets(4, SAMPLES)
  with open(os.path.join(ROOT, "profiles", "puppet_group_latency.json")) as f:
    lat = json.loads(f.readline())
  enq = max(r["group"]["enqueue_ms_median"] for r in lat["runs"] if r["slots"] == 4)
  spin_ms = 400.0
  assert spin_ms >= 20 * enq, (spin_ms, enq)
  g, g2 = _group(), _group()
  rng = np.random.default_rng(2)
  pcm = (0.3 * rng.standard_normal((40, 4, 640))).astype(np.float32)
  ears = {s: np.full((1, 1), 0.005, np.float32) for s in range(4)}
  steady = 0
  for i in range(30):                                   # fill the lookahead; the allocators see every size a steady push needs
    chunk = {s: pcm[i, s] for s in range(4)}
    k = g.audio.ready({s: 640 for s in range(4)})
    e = {s: np.full((k[s], 1), 0.005, np.float32) for s in range(4) if k[s]}
    g.push(chunk, ears=e)
    g2.push(chunk, ears=e)
    steady = steady + 1 if list(k) == [1, 1, 1, 1] else 0
  assert steady >= 5
  cycles = _spin_cycles(spin_ms)
  torch.cuda.synchronize()
  chunk = {s: pcm[30, s] for s in range(4)}
  want = g2.push(chunk, ears=ears)
  want_frames = g2.last_frames.cpu().numpy()
  torch.cuda.synchronize()
  torch.cuda._sleep(cycles)
  ev = torch.cuda.Event()
  ev.record()
  t = time.perf_counter()
  res = g.push(chunk, ears=ears)
  dt = 1000.0 * (time.perf_counter() - t)
  pending = not ev.query()
  print("push returned after %.2f ms with the %.0f ms spin %s" % (dt, spin_ms, "still running" if pending else "ALREADY COMPLETE"))
  assert pending, "push returned after %.1f ms, after the %.0f ms spin ahead of it had completed: it waited for the device (or the host is too slow to tell)" % (dt, spin_ms)
  assert dt < spin_ms / 2, dt
  torch.cuda.synchronize()
  assert {s: [i for i, _ in v] for s, v in res.items()} == {s: [i for i, _ in v] for s, v in want.items()}
  assert all(len(v) == 1 for v in res.values())
  assert np.array_equal(g.last_frames.cpu().numpy(), want_frames)


def _jpgs(d):
  from PIL import Image
  names = sorted(os.listdir(d), key=lambda f: int(f.split(".")[0]))
  assert names == ["%d.jpg" % i for i in range(len(names))], (d, names)
  return np.stack([np.asarray(Image.open(os.path.join(d, f))) for f in names])


def test_infer_streams_cli_matches_infer_stream_per_talker(tmp_path, monkeypatch):
  """infer_streams.main on a 3-line list (two talkers with coefficient files, one without; 13, 30 and 51 frames) writes, per talker, the
  JPEG files of an infer_stream.main run on that talker alone under the same seed: the same count, decoded pixels under the rule of
  test_group_equals_talkers_alone."""
  from voicepuppet_amd.pixrefer import infer_stream, infer_streams
  monkeypatch.chdir(tmp_path)
  _assets(3, SAMPLES[:3])
  with open("talkers.txt", "w") as f:
    f.write("face0.jpg a0.wav photo0.npz\nface1.jpg a1.wav\n\nface2.jpg a2.wav photo2.npz\n")
  infer_streams.main(["--config_path", CFG, "--frame_batch", "4", "--chunk_ms", "130", "--seed", "7", "--output_dir", "many", "talkers.txt"])
  for s, npz in enumerate(("photo0.npz", None, "photo2.npz")):
    np.random.seed(7)
    args = ["--config_path", CFG, "--frame_batch", "4", "--chunk_ms", "130", "--output_dir", "one%d" % s]
    infer_stream.main(args + (["--bfmcoeff", npz] if npz else []) + ["face%d.jpg" % s, "a%d.wav" % s])
    want, got = _jpgs("one%d" % s), _jpgs(os.path.join("many", str(s)))
    assert got.shape == want.shape and got.shape[0] == FRAMES[s], (s, got.shape, want.shape)
    _compare_generated(None, None, got, want, "talker %d" % s)
