"""Event files of voicepuppet_amd/utils/tb_events.py read back by two readers that share nothing with the writer: a TFRecord / protobuf
wire parser written here, and (when google.protobuf imports) Event / Summary message types built from a FileDescriptorProto declared
here after tensorflow's event.proto and summary.proto."""
import io
import os
import re
import socket
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref  # noqa: E402


# ---- an independent CRC-32C and reader ----------------------------------------------------------------------------------------------------
def crc32c_bitwise(data):
  c = 0xFFFFFFFF
  for b in data:
    c ^= b
    for _ in range(8):
      c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
  return c ^ 0xFFFFFFFF


def masked(c):
  return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def records(raw):
  at, out = 0, []
  while at < len(raw):
    n, = struct.unpack("<Q", raw[at:at + 8])
    assert struct.unpack("<I", raw[at + 8:at + 12])[0] == masked(crc32c_bitwise(raw[at:at + 8]))
    data = raw[at + 12:at + 12 + n]
    assert len(data) == n
    assert struct.unpack("<I", raw[at + 12 + n:at + 16 + n])[0] == masked(crc32c_bitwise(data))
    out.append(data)
    at += 16 + n
  assert at == len(raw)
  return out


def fields(buf):
  """-> [(field number, wire type, value)]: varints as ints, 64 / 32 bit as raw bytes, length-delimited as bytes"""
  at, out = 0, []

  def varint():
    nonlocal at
    v = s = 0
    while True:
      b = buf[at]
      at += 1
      v |= (b & 0x7F) << s
      s += 7
      if not b & 0x80:
        return v
  while at < len(buf):
    k = varint()
    f, w = k >> 3, k & 7
    if w == 0:
      out.append((f, w, varint()))
    elif w == 1:
      out.append((f, w, buf[at:at + 8]))
      at += 8
    elif w == 5:
      out.append((f, w, buf[at:at + 4]))
      at += 4
    else:
      assert w == 2
      n = varint()
      out.append((f, w, buf[at:at + n]))
      at += n
  assert at == len(buf)
  return out


def parse_event(data):
  ev = {"summary": []}
  for f, w, v in fields(data):
    if (f, w) == (1, 1):
      ev["wall_time"] = struct.unpack("<d", v)[0]
    elif (f, w) == (2, 0):
      ev["step"] = v
    elif (f, w) == (3, 2):
      ev["file_version"] = v.decode()
    elif (f, w) == (5, 2):
      for f2, w2, value in fields(v):
        assert (f2, w2) == (1, 2)
        item = {}
        for f3, w3, x in fields(value):
          if (f3, w3) == (1, 2):
            item["tag"] = x.decode()
          elif (f3, w3) == (2, 5):
            item["simple_value"] = struct.unpack("<f", x)[0]
          elif (f3, w3) == (4, 2):
            img = dict(((f4, w4), y) for f4, w4, y in fields(x))
            item["image"] = (img[(1, 0)], img[(2, 0)], img[(3, 0)], img[(4, 2)])
          else:
            raise AssertionError((f3, w3))
        ev["summary"].append(item)
    else:
      raise AssertionError((f, w))
  return ev


def protobuf_types():
  """Event and Summary as protobuf sees them, from a descriptor declared here (tensorflow/core/util/event.proto, framework/summary.proto:
  the fields this project writes)."""
  from google.protobuf import descriptor_pb2, descriptor_pool
  try:
    from google.protobuf import message_factory
    get = getattr(message_factory, "GetMessageClass", None)
  except ImportError:
    get = None
  F = descriptor_pb2.FieldDescriptorProto
  fd = descriptor_pb2.FileDescriptorProto(name="vp_test_event.proto", package="vptest", syntax="proto3")

  def message(parent, name, spec):
    m = parent.add()
    m.name = name
    for fname, number, ftype, label, type_name in spec:
      f = m.field.add()
      f.name, f.number, f.type, f.label = fname, number, ftype, label
      if type_name:
        f.type_name = type_name
    return m
  one, many = F.LABEL_OPTIONAL, F.LABEL_REPEATED
  s = message(fd.message_type, "Summary", [("value", 1, F.TYPE_MESSAGE, many, ".vptest.Summary.Value")])
  message(s.nested_type, "Image", [("height", 1, F.TYPE_INT32, one, None), ("width", 2, F.TYPE_INT32, one, None),
                                   ("colorspace", 3, F.TYPE_INT32, one, None), ("encoded_image_string", 4, F.TYPE_BYTES, one, None)])
  message(s.nested_type, "Value", [("tag", 1, F.TYPE_STRING, one, None), ("simple_value", 2, F.TYPE_FLOAT, one, None),
                                   ("image", 4, F.TYPE_MESSAGE, one, ".vptest.Summary.Image")])
  message(fd.message_type, "Event", [("wall_time", 1, F.TYPE_DOUBLE, one, None), ("step", 2, F.TYPE_INT64, one, None),
                                     ("file_version", 3, F.TYPE_STRING, one, None), ("summary", 5, F.TYPE_MESSAGE, one, ".vptest.Summary")])
  pool = descriptor_pool.DescriptorPool()
  pool.Add(fd)
  desc = pool.FindMessageTypeByName("vptest.Event")
  if get is not None:
    return get(desc)
  return message_factory.MessageFactory(pool).GetPrototype(desc)


def small_png(seed, shape=(6, 9, 3)):
  img = np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)
  return img, png_ref.encode(img)


def write_file(tmp_path):
  from voicepuppet_amd.utils.tb_events import EventFileWriter
  w = EventFileWriter(str(tmp_path / "log" / "summary"), wall_time=1700000000.25)
  imgs = {"outputs_summary/outputs/image/%d" % i: small_png(i) for i in range(2)}
  imgs["alphas_summary/alphas/image/0"] = small_png(9, (5, 4))
  w.add_summary(100, {"discriminator_loss": 1.25, "generator_loss_GAN": 0.1, "generator_loss_L1": 3.0e-3},
                {k: (v[0].shape[0], v[0].shape[1], 3 if v[0].ndim == 3 else 1, v[1]) for k, v in imgs.items()}, wall_time=1700000001.5)
  w.add_summary(-1, {"discriminator_loss": float("inf")})
  w.add_summary(1 << 40, None, None, wall_time=3.0)
  w.flush()
  mid = open(w.path, "rb").read()
  w.close()
  w.close()
  with pytest.raises(ValueError):
    w.add_summary(1, {"x": 1.0})
  assert open(w.path, "rb").read() == mid
  return w.path, imgs


def test_file_name_framing_and_contents(tmp_path):
  from PIL import Image
  path, imgs = write_file(tmp_path)
  assert os.path.dirname(path) == str(tmp_path / "log" / "summary")
  assert re.fullmatch(r"events\.out\.tfevents\.1700000000\.%s" % re.escape(socket.gethostname()), os.path.basename(path))
  evs = [parse_event(r) for r in records(open(path, "rb").read())]
  assert len(evs) == 4
  assert evs[0] == {"wall_time": 1700000000.25, "file_version": "brain.Event:2", "summary": []}
  e = evs[1]
  assert e["wall_time"] == 1700000001.5 and e["step"] == 100
  assert [(v["tag"], v["simple_value"]) for v in e["summary"][:3]] == [
      ("discriminator_loss", 1.25), ("generator_loss_GAN", float(np.float32(0.1))), ("generator_loss_L1", float(np.float32(3.0e-3)))]
  assert [v["tag"] for v in e["summary"][3:]] == list(imgs)
  for v in e["summary"][3:]:
    img, data = imgs[v["tag"]]
    h, w, cs, payload = v["image"]
    assert (h, w, cs) == (img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1) and payload == data
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(payload))), img)
  assert evs[2]["step"] == (1 << 64) - 1 and evs[2]["summary"][0]["simple_value"] == float("inf")      # int64 -1 on the wire
  assert evs[3]["step"] == 1 << 40 and evs[3]["summary"] == [] and evs[3]["wall_time"] == 3.0


def test_protobuf_reads_every_record(tmp_path):
  pytest.importorskip("google.protobuf")
  Event = protobuf_types()
  path, imgs = write_file(tmp_path)
  evs = []
  for r in records(open(path, "rb").read()):
    e = Event()
    e.ParseFromString(r)
    assert e.SerializeToString() == r                    # nothing unknown dropped, nothing reordered
    evs.append(e)
  assert evs[0].file_version == "brain.Event:2" and evs[0].wall_time == 1700000000.25 and len(evs[0].summary.value) == 0
  assert evs[1].step == 100 and [v.tag for v in evs[1].summary.value] == ["discriminator_loss", "generator_loss_GAN", "generator_loss_L1"] + list(imgs)
  assert [v.simple_value for v in evs[1].summary.value[:3]] == [1.25, float(np.float32(0.1)), float(np.float32(3.0e-3))]
  for v in evs[1].summary.value[3:]:
    img, data = imgs[v.tag]
    assert (v.image.height, v.image.width, v.image.colorspace) == (img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1)
    assert v.image.encoded_image_string == data
  assert evs[2].step == -1 and evs[3].step == 1 << 40


def test_module_imports_no_tensorflow_tensorboard_or_protobuf():
  src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voicepuppet_amd", "utils", "tb_events.py")).read()
  assert not re.search(r"^\s*(import|from)\s+(tensorflow|tensorboard|google)", src, flags=re.M)
