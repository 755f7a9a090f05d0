"""TensorBoard event files in plain Python - no TensorFlow, tensorboard or protobuf.

What tf.summary.FileWriter('log/summary_pixrefer') and the merged summary op write in the reference (train_pixrefer.py:101-132, 146):
a file events.out.tfevents.<seconds>.<hostname> of TFRecord records, each one serialised Event:

  record     uint64 length | uint32 masked_crc32c(the 8 length bytes) | data | uint32 masked_crc32c(data)        (little endian)
  Event      wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5 (Summary)
  Summary    value = 1 (repeated Summary.Value)
  Value      tag = 1 (string), simple_value = 2 (float), image = 4 (Summary.Image)
  Image      height = 1, width = 2, colorspace = 3 (int32; 1 grey, 3 RGB, 4 RGBA), encoded_image_string = 4 (bytes: a PNG file)

The first record is Event{wall_time, file_version = "brain.Event:2"}.  No graph event is written: there is no graph.  The field numbers
are those of tensorflow/core/util/event.proto and tensorflow/core/framework/summary.proto, restated from the published files.

UNPINNED BY TENSORBOARD: no TensorBoard has read a file this module wrote; it is not installed where this is built.  What pins it: the
record framing and CRC-32C shared with utils/tf_checkpoint.py, and tests/test_tb_events_host.py, which reads the files back with a
parser of its own and with protobuf message types built from a descriptor declared in the test.
"""
import os
import socket
import struct
import time

from .tf_checkpoint import crc32c, crc32c_fast, mask_crc

FILE_VERSION = "brain.Event:2"


def _varint(v):
  v &= (1 << 64) - 1              # a negative int64 is its 64-bit two's complement: ten bytes
  out = bytearray()
  while v >= 0x80:
    out.append((v & 0x7F) | 0x80)
    v >>= 7
  out.append(v)
  return bytes(out)


def _key(field, wire):
  return _varint((field << 3) | wire)


def _bytes_field(field, data):
  return _key(field, 2) + _varint(len(data)) + bytes(data)


def _int_field(field, v):
  return _key(field, 0) + _varint(int(v))


def image_proto(height, width, colorspace, png_bytes):
  return _int_field(1, height) + _int_field(2, width) + _int_field(3, colorspace) + _bytes_field(4, png_bytes)


def summary_proto(scalars=None, images=None):
  """scalars: {tag: number}; images: {tag: (height, width, colorspace, png bytes)} -> a serialised Summary, the values in dict order."""
  out = []
  for tag, v in (scalars or {}).items():
    out.append(_bytes_field(1, _bytes_field(1, tag.encode()) + _key(2, 5) + struct.pack("<f", float(v))))
  for tag, (h, w, cs, png) in (images or {}).items():
    out.append(_bytes_field(1, _bytes_field(1, tag.encode()) + _bytes_field(4, image_proto(h, w, cs, png))))
  return b"".join(out)


def event_proto(wall_time, step=None, file_version=None, summary=None):
  out = _key(1, 1) + struct.pack("<d", float(wall_time))
  if step is not None:
    out += _int_field(2, step)
  if file_version is not None:
    out += _bytes_field(3, file_version.encode())
  if summary is not None:
    out += _bytes_field(5, summary)
  return out


def record(data):
  head = struct.pack("<Q", len(data))
  return head + struct.pack("<I", mask_crc(crc32c(head))) + data + struct.pack("<I", mask_crc(crc32c_fast(data)))


class EventFileWriter:
  """EventFileWriter(logdir) creates logdir/events.out.tfevents.<10-digit seconds>.<hostname> and writes the version event;
  add_summary writes one Event per call."""

  def __init__(self, logdir, wall_time=None):
    os.makedirs(logdir, exist_ok=True)
    now = time.time() if wall_time is None else float(wall_time)
    self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(now), socket.gethostname()))
    self._f = open(self.path, "ab")
    self._f.write(record(event_proto(now, file_version=FILE_VERSION)))
    self._f.flush()

  def add_summary(self, step, scalars=None, images=None, wall_time=None):
    if self._f is None:
      raise ValueError("add_summary on a closed EventFileWriter")
    now = time.time() if wall_time is None else float(wall_time)
    self._f.write(record(event_proto(now, step=int(step), summary=summary_proto(scalars, images))))

  def flush(self):
    if self._f is not None:
      self._f.flush()

  def close(self):
    if self._f is not None:
      self._f.close()
      self._f = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass
