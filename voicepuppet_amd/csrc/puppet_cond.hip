// Frames for stream groups (vp_puppet_*): what lies between a group push's packed expression coefficients and the generator's three
// input tensors, for rows of several talkers at once, without a host wait.
//
//   vp_puppet_splice     infer_bfmvid.splice_coeff (reference infer_bfmvid.py:223-224) per row: photo coefficients of the row's slot
//                        with 80:144 replaced by the streamed expression.  Pure copies.
//   vp_puppet_condition  one launch that writes `inputs` [B,H,H,6], `fg_inputs` [B,H,H,3] and `targets` [B,H,H,3] for B rows: the
//                        channel swap / cv2.resize / paste of render_face (infer_bfmvid.py:110-121; csrc/resize.hip is its uint8 form),
//                        the caller's second swap (:233), the float conversion, the reference panels (:200-203, :229-230) and the
//                        background target by global frame index (:236-238).
//
// Everything before the float conversion is the integer arithmetic of resize_paste_kernel.  The conversion itself has two forms, because
// the two expressions it replaces round differently, and each is reproduced bit for bit from a 256-entry table that every block fills:
//   targets   numpy's float32(u8) / 255.0 (ImageLoader.get_data): a correctly rounded IEEE division.  This translation unit is built with
//             -ffp-contract=off and no fast-math option (csrc/Makefile), and hipcc's default for f32 division is the correctly rounded
//             sequence (v_div_scale / v_div_fmas / v_div_fixup).
//   face      torch's `u8.to(float32) / 255.0` on the device, which divides by a scalar as a multiplication with float32(1 / 255): one ulp
//             away from the division for some of the 256 values.  tests/test_gpu_puppet_group.py compares both against their sources.
//
// The kernel is a streaming one (48 bytes written per pixel, a few read): a wave owns one image line of one row at a time and writes it
// as consecutive 1 KB runs (lane l stores the l-th float4 of the run), so every store instruction of a wave is one contiguous kilobyte on
// all three layouts ([..,6] and [..,3] lines are multiples of 16 bytes long because the image size is a multiple of 256).  What a line
// holds (reference panel, copy, 2x reduction, bilinear, or nothing of the face) is decided once per line and is uniform in the wave.
// The grid is sized to residency and strides over the lines.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "workspace.h"

#pragma clang fp contract(off)

namespace vp {

struct PuppetTab { int ofs; short a0, a1; };     // = ResizeTab of resize.hip (source index, the two 11-bit coefficients)

enum PuppetKind { PK_EMPTY = 0, PK_PANEL = 1, PK_COPY = 2, PK_HALF = 3, PK_LINEAR = 4 };

struct PuppetSlot {        // device copy of a slot's geometry, written at attach
  int kind;                // PK_EMPTY: not attached; PK_PANEL: no coefficients, channels 3:6 are the reference panel
  int side, y0, x0;        // the face is resized to side x side and pasted at rows y0.., columns x0.. of the canvas
  int pad[4];
};

struct CondArgs {
  const PuppetSlot* slots;          // [S]
  const PuppetTab* tabs;            // [S][2 * max_side]: columns, then rows
  const int* row1;                  // [S][max_side]
  const float* refer;               // [S][H][H][3]
  const float* fg;                  // [S][H][H][3]
  const unsigned char* faces;       // [n_faces][fs][fs][3], rasteriser order
  const unsigned char* bank;        // [n_bg][H][H][3]
  const int* rows;                  // [B][4]: slot, face row or -1, background row or -1, global frame index (not read here)
  float* inputs; float* fg_inputs; float* targets;
  int S, B, H, fs, max_side, n_faces, n_bg;
};

template <int KIND>
__device__ __forceinline__ int face_u8(const CondArgs& a, const PuppetSlot& s, const unsigned char* src, const PuppetTab* xt, PuppetTab yt, int r1,
                                       int dy, int x, int c) {
  const int dx = x - s.x0;
  if (dx < 0 || dx >= s.side) return 0;                   // the zero canvas beside the pasted image
  const int ws = a.fs;
  if (KIND == PK_COPY) return src[(dy * ws + dx) * 3 + c];
  if (KIND == PK_HALF) {
    const unsigned char* p = src + ((2 * dy) * ws + 2 * dx) * 3 + c;
    return (p[0] + p[3] + p[ws * 3] + p[ws * 3 + 3] + 2) >> 2;
  }
  const PuppetTab t = xt[dx];
  const int x1 = t.a1 ? t.ofs + 1 : t.ofs;
  const unsigned char* p0 = src + yt.ofs * ws * 3;
  const unsigned char* p1 = src + r1 * ws * 3;
  const int d0 = p0[t.ofs * 3 + c] * t.a0 + p0[x1 * 3 + c] * t.a1;
  const int d1 = p1[t.ofs * 3 + c] * t.a0 + p1[x1 * 3 + c] * t.a1;
  return ((((int)yt.a0 * (d0 >> 4)) >> 16) + (((int)yt.a1 * (d1 >> 4)) >> 16) + 2) >> 2;
}

// the `inputs` line: channels 0:3 the reference panel, 3:6 the face (KIND) as float
template <int KIND>
__device__ __forceinline__ void inputs_line(const CondArgs& a, const PuppetSlot& s, const float* lut, const float* refer_line, const unsigned char* src,
                                            const PuppetTab* xt, PuppetTab yt, int r1, int dy, float* out_line, int lane) {
  const int nq = a.H * 6 / 4;
  for (int q = lane; q < nq; q += 64) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = 4 * q + j, x = f / 6, c = f - 6 * x;
      if (c < 3) v[j] = refer_line[x * 3 + c];
      else if (KIND == PK_PANEL) v[j] = refer_line[x * 3 + c - 3];
      else if (KIND == PK_EMPTY) v[j] = lut[0];
      else v[j] = lut[face_u8<KIND>(a, s, src, xt, yt, r1, dy, x, c - 3)];
    }
    reinterpret_cast<float4*>(out_line)[q] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__global__ __launch_bounds__(256) void puppet_condition_kernel(const CondArgs a) {
  __shared__ float lut[256], lut_face[256];
  lut[threadIdx.x] = (float)(int)threadIdx.x / 255.0f;                  // numpy: float32(u8) / 255.0, correctly rounded
  lut_face[threadIdx.x] = (float)(int)threadIdx.x * (1.0f / 255.0f);    // torch: u8.to(float32) / 255.0 = x * float32(1 / 255)
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const int H = a.H;
  const size_t plane = (size_t)H * H;
  for (int line = wave; line < a.B * H; line += nwaves) {
    const int b = line / H, y = line - b * H;
    const int slot = a.rows[4 * b], face = a.rows[4 * b + 1], bg = a.rows[4 * b + 2];
    if (slot < 0 || slot >= a.S || face >= a.n_faces || bg >= a.n_bg) continue;      // a table this launch cannot serve writes nothing
    const PuppetSlot s = a.slots[slot];
    if (s.kind == PK_EMPTY || (s.kind != PK_PANEL && face < 0)) continue;
    const size_t lo = ((size_t)b * H + y) * H, so = ((size_t)slot * H + y) * H;
    // inputs
    {
      const float* refer_line = a.refer + so * 3;
      float* out_line = a.inputs + lo * 6;
      const int dy = y - s.y0;
      const int kind = s.kind == PK_PANEL ? PK_PANEL : ((dy < 0 || dy >= s.side) ? PK_EMPTY : s.kind);
      const unsigned char* src = a.faces + (size_t)(face < 0 ? 0 : face) * a.fs * a.fs * 3;
      const PuppetTab* xt = a.tabs + (size_t)slot * 2 * a.max_side;
      PuppetTab yt = {0, 0, 0};
      int r1 = 0;
      if (kind == PK_LINEAR) { yt = xt[a.max_side + dy]; r1 = a.row1[(size_t)slot * a.max_side + dy]; }
      switch (kind) {                                           // uniform in the wave
        case PK_PANEL: inputs_line<PK_PANEL>(a, s, lut_face, refer_line, src, xt, yt, r1, dy, out_line, lane); break;
        case PK_COPY: inputs_line<PK_COPY>(a, s, lut_face, refer_line, src, xt, yt, r1, dy, out_line, lane); break;
        case PK_HALF: inputs_line<PK_HALF>(a, s, lut_face, refer_line, src, xt, yt, r1, dy, out_line, lane); break;
        case PK_LINEAR: inputs_line<PK_LINEAR>(a, s, lut_face, refer_line, src, xt, yt, r1, dy, out_line, lane); break;
        default: inputs_line<PK_EMPTY>(a, s, lut_face, refer_line, src, xt, yt, r1, dy, out_line, lane); break;
      }
    }
    const int nq = H * 3 / 4;
    // fg_inputs: the slot's foreground panel
    {
      const float4* p = reinterpret_cast<const float4*>(a.fg + so * 3);
      float4* o = reinterpret_cast<float4*>(a.fg_inputs + lo * 3);
      for (int q = lane; q < nq; q += 64) o[q] = p[q];
    }
    // targets: the background of the row's global frame index, or 0.5
    {
      float4* o = reinterpret_cast<float4*>(a.targets + lo * 3);
      if (bg >= 0) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(a.bank + ((size_t)bg * plane + (size_t)y * H) * 3);
        for (int q = lane; q < nq; q += 64) {
          const uint32_t u = p[q];
          o[q] = make_float4(lut[u & 255u], lut[(u >> 8) & 255u], lut[(u >> 16) & 255u], lut[u >> 24]);
        }
      } else {
        for (int q = lane; q < nq; q += 64) o[q] = make_float4(0.5f, 0.5f, 0.5f, 0.5f);
      }
    }
  }
}

// out[r][j] = j in [80,144) ? expr[src(r)][j - 80] : photo[slot(r)][j]
__global__ __launch_bounds__(256) void puppet_splice_kernel(const float* __restrict__ photo, const float* __restrict__ expr, const int* __restrict__ rows,
                                                            float* __restrict__ out, int R, int S, int K) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R * 257) return;
  const int r = i / 257, j = i - r * 257;
  const int slot = rows[4 * r], k = rows[4 * r + 1];
  if (slot < 0 || slot >= S || k < 0 || k >= K) return;
  out[i] = (j >= 80 && j < 144) ? expr[(size_t)k * 64 + j - 80] : photo[(size_t)slot * 257 + j];
}

}  // namespace vp

struct vp_puppet {
  vp_puppet_desc d;
  int max_side;
  vp::PuppetSlot* slots_dev;
  float *coeff, *refer, *fg;
  vp::PuppetTab* tabs;
  int* row1;
  std::vector<vp::PuppetSlot> slots;
  const unsigned char* bank;
  int n_bg;
};

using namespace vp;

static int puppet_check(const vp_puppet_desc* d, vp_puppet* h) {
  if (const int rc = check_desc(d, "vp_puppet")) return rc;
  if (d->slots < 1 || d->slots > VP_PUPPET_MAX_SLOTS) { set_err("vp_puppet: bad descriptor (slots %d, 1 .. %d)", d->slots, VP_PUPPET_MAX_SLOTS); return VP_ERR_ARG; }
  if (d->frame_batch < 1 || d->frame_batch > 1024) { set_err("vp_puppet: bad descriptor (frame_batch %d, 1 .. 1024)", d->frame_batch); return VP_ERR_ARG; }
  if (d->img_size < 256 || d->img_size % 256) { set_err("vp_puppet: bad descriptor (img_size %d is not a multiple of 256)", d->img_size); return VP_ERR_ARG; }
  if (d->face_size < 2 || d->face_size > 4096) { set_err("vp_puppet: bad descriptor (face_size %d, 2 .. 4096)", d->face_size); return VP_ERR_ARG; }
  // offsets inside one image, one face and one slot's tables are 32-bit in the kernel (rows and slots are widened)
  if (d->img_size > 4096) { set_err("vp_puppet: bad descriptor (img_size %d: offsets inside an image would leave 32-bit lane offsets)", d->img_size); return VP_ERR_ARG; }
  h->d = *d;
  h->max_side = 4 * d->img_size;
  return VP_OK;
}

static size_t puppet_carve(vp_puppet* h, void* base) {
  Arena ar(base);
  const size_t S = h->d.slots, px = (size_t)h->d.img_size * h->d.img_size;
  h->slots_dev = ar.take<PuppetSlot>(S);
  h->coeff = ar.take<float>(S * 257);
  h->tabs = ar.take<PuppetTab>(S * 2 * h->max_side);
  h->row1 = ar.take<int>(S * h->max_side);
  h->refer = ar.take<float>(S * px * 3);
  h->fg = ar.take<float>(S * px * 3);
  return align256(ar.total());
}

extern "C" {

size_t vp_puppet_desc_size(void) { return sizeof(vp_puppet_desc); }

size_t vp_puppet_workspace_bytes(const vp_puppet_desc* d) {
  vp_puppet h;
  return puppet_check(d, &h) ? 0 : puppet_carve(&h, nullptr);
}

int vp_puppet_create(const vp_puppet_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_puppet_t** out) {
  // (a short workspace is VP_ERR_ARG here, VP_ERR_WORKSPACE in every other family: callers may test for the code, so it stays)
  if (const int rc = open_handle("vp_puppet_create", d, puppet_check, puppet_carve, workspace, workspace_bytes, out, VP_ERR_ARG)) return rc;
  vp_puppet* h = *out;
  h->slots.assign(d->slots, PuppetSlot{});
  h->bank = nullptr; h->n_bg = 0;
  // every slot empty, no coefficients: the slot table and the coefficients, up to where the tables start
  const hipError_t e = hipMemsetAsync(h->slots_dev, 0, (size_t)((char*)h->tabs - (char*)h->slots_dev), (hipStream_t)stream);
  if (e != hipSuccess) { set_err("vp_puppet_create: hipMemsetAsync -> %s", hipGetErrorString(e)); delete h; *out = nullptr; return VP_ERR_HIP; }
  return VP_OK;
}

void vp_puppet_destroy(vp_puppet_t* h) { delete h; }

int vp_puppet_attach(vp_puppet_t* h, int slot, const float* refer, const float* fg_refer, const float* photo_coeff, int side, int y0, int x0,
                     void* stream) {
  if (!h || slot < 0 || slot >= h->d.slots || !refer || !fg_refer) { set_err("vp_puppet_attach: bad argument"); return VP_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const int fs = h->d.face_size, ms = h->max_side, H = h->d.img_size;
  PuppetSlot s{};
  if (!photo_coeff) {
    s.kind = PK_PANEL;
  } else {
    if (side < 1 || side > ms) { set_err("vp_puppet_attach: face side %d outside 1 .. %d", side, ms); return VP_ERR_ARG; }
    if (y0 < -ms || y0 > H || x0 < -ms || x0 > H) { set_err("vp_puppet_attach: paste offset (%d, %d) nowhere near the canvas", y0, x0); return VP_ERR_ARG; }
    s.kind = side == fs ? PK_COPY : (fs == 2 * side ? PK_HALF : PK_LINEAR);
    s.side = side; s.y0 = y0; s.x0 = x0;
  }
  const size_t px = (size_t)H * H * 3;
  // attach is not a push: it may wait (pageable sources), once per talker
  if (s.kind == PK_LINEAR) {
    std::vector<int> ofs(side), r1(side);
    std::vector<short> a0(side), a1(side);
    std::vector<PuppetTab> tab((size_t)2 * side);
    int rc = vp_resize_linear_table(fs, side, 0, ofs.data(), a0.data(), a1.data(), nullptr);
    if (rc) return rc;
    for (int i = 0; i < side; ++i) tab[i] = PuppetTab{ofs[i], a0[i], a1[i]};
    rc = vp_resize_linear_table(fs, side, 1, ofs.data(), a0.data(), a1.data(), r1.data());
    if (rc) return rc;
    for (int i = 0; i < side; ++i) tab[side + i] = PuppetTab{ofs[i], a0[i], a1[i]};
    PuppetTab* dt = h->tabs + (size_t)slot * 2 * ms;
    VP_HIP_CHECK(hipMemcpyAsync(dt, tab.data(), side * sizeof(PuppetTab), hipMemcpyHostToDevice, st));
    VP_HIP_CHECK(hipMemcpyAsync(dt + ms, tab.data() + side, side * sizeof(PuppetTab), hipMemcpyHostToDevice, st));
    VP_HIP_CHECK(hipMemcpyAsync(h->row1 + (size_t)slot * ms, r1.data(), side * sizeof(int), hipMemcpyHostToDevice, st));
    VP_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (photo_coeff)
    VP_HIP_CHECK(hipMemcpyAsync(h->coeff + (size_t)slot * 257, photo_coeff, 257 * sizeof(float), hipMemcpyHostToDevice, st));
  else
    VP_HIP_CHECK(hipMemsetAsync(h->coeff + (size_t)slot * 257, 0, 257 * sizeof(float), st));
  VP_HIP_CHECK(hipMemcpyAsync(h->refer + (size_t)slot * px, refer, px * sizeof(float), hipMemcpyDeviceToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(h->fg + (size_t)slot * px, fg_refer, px * sizeof(float), hipMemcpyDeviceToDevice, st));
  VP_HIP_CHECK(hipMemcpyAsync(h->slots_dev + slot, &s, sizeof(s), hipMemcpyHostToDevice, st));
  VP_HIP_CHECK(hipStreamSynchronize(st));
  h->slots[slot] = s;
  return VP_OK;
}

int vp_puppet_set_backgrounds(vp_puppet_t* h, const unsigned char* bank, int count) {
  if (!h || count < 0 || (count > 0 && !bank)) { set_err("vp_puppet_set_backgrounds: bad argument"); return VP_ERR_ARG; }
  h->bank = bank; h->n_bg = count;
  return VP_OK;
}

int vp_puppet_splice(vp_puppet_t* h, const float* expr, int expr_rows, const int* rows, int count, float* coeff_out, void* stream) {
  if (!h || !expr || !rows || !coeff_out || count < 1 || expr_rows < 1 || count > (1 << 22)) { set_err("vp_puppet_splice: bad argument"); return VP_ERR_ARG; }
  hipLaunchKernelGGL(puppet_splice_kernel, dim3((count * 257 + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     h->coeff, expr, rows, coeff_out, count, h->d.slots, expr_rows);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_puppet_condition(vp_puppet_t* h, const unsigned char* faces, int face_rows, const int* rows, int count, float* inputs, float* fg_inputs,
                        float* targets, void* stream) {
  if (!h || !rows || !inputs || !fg_inputs || !targets || count < 1 || count > h->d.frame_batch || face_rows < 0 || (face_rows > 0 && !faces)) {
    set_err("vp_puppet_condition: bad argument (1 .. frame_batch rows, device tables and tensors)");
    return VP_ERR_ARG;
  }
  CondArgs a{};
  a.slots = h->slots_dev;
  a.tabs = h->tabs;
  a.row1 = h->row1;
  a.refer = h->refer;
  a.fg = h->fg;
  a.faces = faces; a.bank = h->bank; a.rows = rows;
  a.inputs = inputs; a.fg_inputs = fg_inputs; a.targets = targets;
  a.S = h->d.slots; a.B = count; a.H = h->d.img_size; a.fs = h->d.face_size; a.max_side = h->max_side; a.n_faces = face_rows; a.n_bg = h->n_bg;
  // one wave per image line; 256 CUs x 2 blocks of 4 waves keep every CU streaming without a tail of tiny blocks
  int blocks = (count * a.H + 3) / 4;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(puppet_condition_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  VP_HIP_CHECK(hipGetLastError());
  return VP_OK;
}

int vp_puppet_tensor(vp_puppet_t* h, const char* name, void** ptr, int64_t shape[4]) {
  if (!h || !name || !ptr) { set_err("vp_puppet_tensor: bad argument"); return VP_ERR_ARG; }
  const std::string n(name);
  const int64_t S = h->d.slots, H = h->d.img_size;
  int64_t shp[4] = {S, 1, 1, 1};
  if (n == "coeff") { *ptr = h->coeff; shp[1] = 257; }
  else if (n == "refer") { *ptr = h->refer; shp[1] = H; shp[2] = H; shp[3] = 3; }
  else if (n == "fg") { *ptr = h->fg; shp[1] = H; shp[2] = H; shp[3] = 3; }
  else { set_err("vp_puppet_tensor: no tensor '%s' (coeff, refer, fg)", name); return VP_ERR_ARG; }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = shp[i];
  return VP_OK;
}

int vp_puppet_slot_info(const vp_puppet_t* h, int slot, int info[4]) {
  if (!h || !info || slot < 0 || slot >= h->d.slots) { set_err("vp_puppet_slot_info: bad argument"); return VP_ERR_ARG; }
  const PuppetSlot& s = h->slots[slot];
  info[0] = s.kind; info[1] = s.side; info[2] = s.y0; info[3] = s.x0;
  return VP_OK;
}

}  // extern "C"
