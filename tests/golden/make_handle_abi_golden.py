"""Records tests/golden/handle_abi.json: what the C ABI's device-handle families answer before any device call.  Per family, for two valid
descriptors (the smallest it accepts, and the one its host test or wrapper default uses), the bytes of every sizing query; and the return
code with the full vp_last_error() text of three refusals: a null descriptor, struct_bytes - 4, and *_create on a dummy pointer with one
byte less than the need.  tests/test_workspace_host.py runs record() on the library under test and compares with the file, so the file
is made from a build of the commit BEFORE a change to the handles' host code, never from the change itself:

  (build that commit in a second checkout)   VP_LIB=<that checkout>/voicepuppet_amd/libvp_hip.so python tests/golden/make_handle_abi_golden.py

Left out, and why: logmel, bfmnet and pixrefer descriptors have no struct_bytes field, so they have no struct_bytes case.  Every create
below refuses a short workspace before its first device call, the planners' included, so none of the short cases is left out.  The scan
workspace of jpegdec has no create of its own: its short case is vp_jpegdec_enable_scan on a decoder created over a dummy pointer (that
create makes no device call)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from voicepuppet_amd import _lib  # noqa: E402

PATH = os.path.join(HERE, "handle_abi.json")
P = ctypes.c_void_p
FAKE = P(1 << 20)          # never dereferenced by a refusal
F32, BF16 = _lib.VP_F32, _lib.VP_BF16


def _rates(*r):
  return (ctypes.c_int * 8)(*r)


def _sized(cls, *fields):
  return lambda size_delta=0: cls(ctypes.sizeof(cls) + size_delta, *fields)


def _plain(cls, *fields):
  return lambda size_delta=0: cls(*fields)


# family -> (prefix, [descriptor makers: smallest, the host test's], sizing queries [(suffix, extra args)], what create takes between the
# workspace size and the out pointer, whether the descriptor has struct_bytes)
FAMILIES = {
    "jpeg": ("vp_jpeg", [_sized(_lib.JpegDesc, 1, 16, 16, 1), _sized(_lib.JpegDesc, 64, 512, 512, 75)],
             [("workspace_bytes", ()), ("frame_capacity", ())], (None,), True),
    "png": ("vp_png", [_sized(_lib.PngDesc, 1, 1, 1, 1, -1), _sized(_lib.PngDesc, 3, 512, 512, 3, -1)],
            [("workspace_bytes", ()), ("frame_capacity", ()), ("rows_per_strip", ())], (None,), True),
    "jpegdec": ("vp_jpegdec", [_sized(_lib.JpegDecDesc, 1, 1, 1, 1, 1, 0), _sized(_lib.JpegDecDesc, 64, 256, 768, 1 << 20, 4096, 1)],
                [("workspace_bytes", ()), ("scan_workspace_bytes", (32,)), ("scan_workspace_bytes", (128,)), ("scan_workspace_bytes", (4096,))],
                (), True),
    "pcmin": ("vp_pcmin", [_sized(_lib.PcmInDesc, 1, 1000, 1, 1, _rates(1000)), _sized(_lib.PcmInDesc, 4, 16000, 1 << 16, 1, _rates(48000))],
              [("workspace_bytes", ())], (None,), True),
    "frame_metrics": ("vp_frame_metrics", [_sized(_lib.FrameMetricsDesc, 1, 11, 11), _sized(_lib.FrameMetricsDesc, 64, 512, 512)],
                      [("workspace_bytes", ())], (), True),
    "avimux": ("vp_avimux", [_sized(_lib.AviMuxDesc, 1, 1, 1, 0), _sized(_lib.AviMuxDesc, 9, 260, 8, 1921)],
               [("workspace_bytes", ()), ("out_capacity", ()), ("table_bytes", (0,)), ("table_bytes", (1,))], (), True),
    "triptych": ("vp_triptych", [_sized(_lib.TriptychDesc, 1, 11, 2, 11), _sized(_lib.TriptychDesc, 64, 512, 224, 512)],
                 [("workspace_bytes", ())], (None,), True),
    "puppet": ("vp_puppet", [_sized(_lib.PuppetDesc, 1, 1, 256, 2), _sized(_lib.PuppetDesc, 4, 8, 512, 224)],
               [("workspace_bytes", ())], (None,), True),
    "logmel": ("vp_logmel", [_plain(_lib.LogMelDesc, 16000, 1, 16, 1, 16, 80.0, 7600.0, 1, 16),
                             _plain(_lib.LogMelDesc, 16000, 80, 512, 128, 512, 80.0, 7600.0, 1, 4096)],
               [("workspace_bytes", ())], (None,), False),
    "bfmnet": ("vp_bfmnet", [_plain(_lib.BfmNetDesc, 1, 1, 80, F32), _plain(_lib.BfmNetDesc, 4, 25, 80, BF16)],
               [("workspace_bytes", ())], (FAKE, None), False),
    "bfmstream_group": ("vp_bfmstream_group", [_sized(_lib.BfmStreamGroupDesc, 1, 1, 80, F32, 16000, 80.0, 7600.0),
                                               _sized(_lib.BfmStreamGroupDesc, 4, 1, 80, F32, 16000, 80.0, 7600.0)],
                        [("workspace_bytes", ())], (FAKE, None), True),
    "pixrefer": ("vp_pixrefer", [_plain(_lib.PixReferDesc, 1, 256, 8, 8, F32, 0, 500.0, 1.0, 0),
                                 _plain(_lib.PixReferDesc, 1, 256, 64, 64, BF16, 1, 500.0, 1.0, 0)],
                 [("workspace_bytes", ())], (FAKE, FAKE, FAKE, FAKE, FAKE, None), False),
}


def record(L):
  """{family: {"sizes": [...], "refusals": [...]}} of the library L (voicepuppet_amd._lib.lib())."""
  def err():
    return L.vp_last_error().decode()

  out = {}
  for family, (prefix, makers, queries, create_args, has_size) in FAMILIES.items():
    fn = lambda suffix: getattr(L, "%s_%s" % (prefix, suffix))
    sizes = []
    for k, make in enumerate(makers):
      d = make()
      sizes.append({"descriptor": k, "values": {"%s%s" % (s, list(extra) if extra else ""): int(fn(s)(ctypes.byref(d), *extra)) for s, extra in queries}})
      assert sizes[-1]["values"]["workspace_bytes"] > 0, (family, k, err())
    cases = [("null", None)] + ([("struct_bytes - 4", makers[0](-4))] if has_size else [])
    refusals = []
    for what, d in cases:
      ref = ctypes.byref(d) if d is not None else None
      for s, extra in queries:
        refusals.append({"case": what, "call": s, "value": int(fn(s)(ref, *extra)), "error": err()})
      h = P()
      rc = fn("create")(ref, FAKE, 1 << 40, *create_args, ctypes.byref(h))
      refusals.append({"case": what, "call": "create", "rc": rc, "error": err(), "out_is_null": h.value is None})
    d = makers[0]()
    need, h = fn("workspace_bytes")(ctypes.byref(d)), P()
    rc = fn("create")(ctypes.byref(d), FAKE, need - 1, *create_args, ctypes.byref(h))
    refusals.append({"case": "one byte short", "call": "create", "rc": rc, "error": err(), "out_is_null": h.value is None})
    if family == "jpegdec":
      assert fn("create")(ctypes.byref(d), FAKE, need, ctypes.byref(h)) == 0, err()
      need = fn("scan_workspace_bytes")(ctypes.byref(d), 32)
      rc = fn("enable_scan")(h, FAKE, need - 1, 32, 8)
      refusals.append({"case": "one byte short", "call": "enable_scan", "rc": rc, "error": err()})
      fn("destroy")(h)
    out[family] = {"sizes": sizes, "refusals": refusals}
  return out


def main():
  got = record(_lib.lib())
  with open(PATH, "w") as f:
    notes = ["logmel, bfmnet and pixrefer descriptors have no struct_bytes field: no 'struct_bytes - 4' case",
             "every create refuses a short workspace before its first device call, the planners' included: no short case is left out",
             "the jpegdec scan workspace has no create: its short case is vp_jpegdec_enable_scan on a decoder created over a dummy pointer"]
    json.dump({"library": "the parent of the commit that introduced csrc/workspace.h", "notes": notes, "families": got}, f, indent=1, sort_keys=True)
    f.write("\n")
  print(PATH, os.path.getsize(PATH), "bytes,", sum(len(v["refusals"]) for v in got.values()), "refusals")


if __name__ == "__main__":
  main()
