"""What every Python wrapper of a libvp_hip.so handle shares (include/vp_hip.h: vp_X_workspace_bytes, vp_X_create, vp_X_tensor,
vp_X_destroy): the pointer and stream arguments, the handle's life cycle, views of named tensors inside its workspace, and the host
read of "byte rows + lengths".  Argument checking of a wrapper's own calls stays with the wrapper, but for the two arguments the image
families (KeyMatte, MatteCleaner, MatteSolver, FrameMetrics) all take, which are checked here rather than in a module of their own:
a batch of RGB frames with its pitch and stride (frame_layout, rgb_frames) and a contiguous uint8 plane (u8_plane).
"""
import ctypes
import math

import torch

from . import _lib


def ptr(t):
  """A tensor's device address for the C ABI; None is a NULL pointer."""
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace_view(workspace, address, shape, dtype):
  """The `dtype` view of `shape` at byte address `address` inside the uint8 tensor `workspace` (no copy).  An address in front of the
  workspace or a view that ends behind it raises: the pointer belongs to another buffer."""
  shape = tuple(int(s) for s in shape)
  nbytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
  off = int(address or 0) - workspace.data_ptr()
  if off < 0 or off + nbytes > workspace.numel():
    raise ValueError("a %s view of %s at offset %d does not lie inside the workspace of %d bytes" % (dtype, shape, off, workspace.numel()))
  return workspace[off:off + nbytes].view(dtype).view(shape)


class Handle:
  """One handle of the library with the workspace it lives in.  A subclass's __init__ builds its descriptor, calls _open and sets its own
  fields; L, desc, workspace and h are what tests and scripts read (and may assign)."""

  def _query(self, prefix, desc, invalid):
    """First half of _open, for a class that has work to do between the size query and the allocation: sets L and desc and returns
    vp_<prefix>_workspace_bytes; a descriptor the library refuses raises ValueError(invalid + the library's reason)."""
    self.L, self.desc, self._prefix = _lib.lib(), desc, prefix
    ws = getattr(self.L, "vp_%s_workspace_bytes" % prefix)(ctypes.byref(desc))
    if ws == 0:
      raise ValueError("%s: %s" % (invalid, self.L.vp_last_error().decode()))
    return ws

  def _create(self, ws, args=(), zero=False, device="cuda"):
    """Second half: allocates the workspace of `ws` bytes (zero-filled or not) and calls vp_<prefix>_create; sets workspace and h."""
    self.workspace = (torch.zeros if zero else torch.empty)(ws, dtype=torch.uint8, device=device)
    h = ctypes.c_void_p()
    create = "vp_%s_create" % self._prefix
    _lib.check(getattr(self.L, create)(ctypes.byref(self.desc), ptr(self.workspace), ws, *args, ctypes.byref(h)), create)
    self.h = h

  def _open(self, prefix, desc, args=(), zero=False, invalid="invalid descriptor", device="cuda"):
    """args: what vp_<prefix>_create takes between the workspace size and the out pointer."""
    self._create(self._query(prefix, desc, invalid), args, zero, device)

  def close(self):
    """Destroys the handle now; a second call does nothing.  A call on a closed handle is an error from the library, not a crash."""
    if getattr(self, "h", None):
      getattr(self.L, "vp_%s_destroy" % self._prefix)(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def _tensor(self, name, dtype, shape, workspace=None):
    """View of the buffer vp_<prefix>_tensor names.  shape: how many of the four extents the library reports form the view, or a
    function of the four.  workspace: the buffer it lies in when that is not self.workspace."""
    p, shp = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
    query = "vp_%s_tensor" % self._prefix
    _lib.check(getattr(self.L, query)(self.h, name.encode(), ctypes.byref(p), shp), query)
    extents = [int(v) for v in shp]
    shape = shape(extents) if callable(shape) else extents[:shape]
    return workspace_view(self.workspace if workspace is None else workspace, p.value, shape, dtype)


def frame_layout(t, who, name="frames"):
  """(row pitch, frame stride) in bytes of a [n, H, W, 3] view whose pixel's values and row's pixels are adjacent and whose rows and
  frames do not overlap; any other view is refused in the name of `who`.  Reads shape and strides only: a CPU tensor will do."""
  n, H, W, _ = t.shape
  e = t.element_size()
  if t.stride(3) != 1 or t.stride(2) != 3 or t.stride(1) < 3 * W or (n > 1 and t.stride(0) < (H - 1) * t.stride(1) + 3 * W):
    raise ValueError("%s: %s has strides %s: a pixel's values and a row's pixels must be adjacent, rows and frames must not overlap"
                     % (who, name, tuple(t.stride())))
  pitch = t.stride(1) * e
  return pitch, max(t.stride(0) * e, (H - 1) * pitch + 3 * W * e)         # a single frame's stride(0) is arbitrary


def rgb_frames(t, who, name="frames"):
  """A device uint8 RGB batch [n, H, W, 3] -> (pitch, stride, n, H, W), pitch and stride as frame_layout gives them."""
  if t.dim() != 4 or t.shape[3] != 3 or t.dtype != torch.uint8 or not t.is_cuda:
    raise ValueError("%s: a device uint8 tensor [n, H, W, 3]" % who)
  return frame_layout(t, who, name) + tuple(int(v) for v in t.shape[:3])


def u8_plane(t, who, name, n=None, H=None, W=None, exact=False, channels=None):
  """Refuses t unless it is a contiguous device uint8 tensor: without n any [n, H, W]; with n, H, W one of [>= n, H, W] (exact: of
  [n, H, W]), with `channels` as a fourth extent when given."""
  tail = () if channels is None else (int(channels),)
  ok = t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.dim() == 3 + len(tail)
  if n is None:
    if not ok:
      raise ValueError("%s: %s must be a contiguous device uint8 tensor [n, H, W]" % (who, name))
  elif not ok or (t.shape[0] != n if exact else t.shape[0] < n) or tuple(t.shape[1:]) != (H, W) + tail:
    raise ValueError("%s: %s must be a contiguous device uint8 [%s%d, %d, %d%s]" % (who, name, "" if exact else ">= ", n, H, W, "".join(", %d" % c for c in tail)))


def rows_to_host(pairs):
  """pairs: [(rows uint8 [K, cap], lengths int32 [K])] on the device -> [(host uint8 array [K, used], host int32 lengths [K])], used the
  longest length of the pair (no row copy when it is 0).  Pinned copies of all the lengths, one wait, pinned copies of the used prefixes,
  one wait.  Negative lengths are handed on as they are."""
  current = torch.cuda.current_stream()
  pinned = []
  for _, lengths in pairs:
    host = torch.empty(lengths.shape, dtype=torch.int32).pin_memory()
    host.copy_(lengths, non_blocking=True)
    pinned.append(host)
  current.synchronize()
  res, copied = [], False
  for (rows, _), host in zip(pairs, pinned):
    n = host.numpy().copy()
    K = int(n.shape[0])
    used = max(int(n.max()), 0) if K else 0
    data = torch.empty(K, used, dtype=torch.uint8)
    if used > 0:
      data = data.pin_memory()
      data.copy_(rows[:K, :used], non_blocking=True)
      copied = True
    res.append((data, n))
  if copied:
    current.synchronize()
  return [(data.numpy(), n) for data, n in res]


def slot_arrays(slots, n_by_slot, finish):
  """The per-slot arguments of a group push or ready query: (c_longlong [slots] counts from {slot: n} or a sequence, c_int [slots] flags
  of the slots in `finish`)."""
  n = (ctypes.c_longlong * slots)()
  fin = (ctypes.c_int * slots)()
  items = n_by_slot.items() if isinstance(n_by_slot, dict) else enumerate(n_by_slot or ())
  for s, v in items:
    n[int(s)] = int(v)
  for s in finish or ():
    fin[int(s)] = 1
  return n, fin


def grow(buf, nbytes, device):
  """`buf` when it holds nbytes, else a new uint8 scratch tensor of nbytes on `device` (the caller keeps what is returned)."""
  if buf is None or buf.numel() < nbytes:
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
  return buf
