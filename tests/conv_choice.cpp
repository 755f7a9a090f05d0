// Prints every plan-time choice of the convolution launch path - kernel, plan family, tile, K split, packed-weight layout - for a
// fixed list of layers, at the default knobs and under every kernel-selecting vp_tune key, and vp_tune's return codes.  A stand-alone
// program (no GPU: it plans, it never launches) that links against the host-only sanitizer build of the library;
// tests/test_conv_choice_host.py compares its output with tests/golden/conv_choice.txt byte for byte.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "conv_ops.h"
#include "vp_hip.h"

using namespace vp;

namespace {

std::vector<std::string> g_lines;      // the lines of the sweep being made
#define EMIT(...) do { char buf_[512]; snprintf(buf_, sizeof(buf_), __VA_ARGS__); g_lines.push_back(buf_); } while (0)

void show(const char* net, const char* layer, const char* what, int N, int bf, const IgemmPlan& p) {
  int bc, bp;
  igemm_tile(p.cfg, &bc, &bp);
  EMIT("%s/%s %s %d %s: %s/%s %d %dx%d %d %d %d%d%d", net, layer, what, N, bf ? "bf16" : "f32", conv_kernel_name(p.a.kern),
       conv_kernel_name(conv_staging(p.a.kern)), p.cfg, bc, bp, p.a.splitk, p.a.CoutPad, p.a.rowperm, p.pack.perm, p.pack.kswap);
}

void show_wgrad(const char* net, const char* layer, int N, int bf, const WgradPlan& w) {
  int bm, bn;
  wgrad_tile(w.cfg, &bm, &bn);
  EMIT("%s/%s wgrad %d %s: %d %dx%d %d %d %d %d", net, layer, N, bf ? "bf16" : "f32", w.cfg, bm, bn, w.a.splitk, w.a.Mpad,
       w.a.Dpad, w.a.fastw);
}

// ---- the three nets of a PixReferNet training step, planned as the step planner plans them ----
struct Lay {
  const char* name;
  int kind, ks, stride, pad;
  int div;            // input side = image side / div (+ off)
  int off;
  int c0, c1;         // channels of the one or two source tensors
  int cin_real, cout;
  bool bn;
  int in_act, out_act;
  bool from_input;    // reads a network input (8 padded channels)
  bool src_relu;      // its source was produced with a relu epilogue
  bool f32_out;
  bool relu_copy;     // first layers: a consumer reads relu(output) as well as lrelu(output)
};
struct NetDesc { const char* name; int mult, groups; bool alt, halves, input_grads; const Lay* l; int nl; };

const int G = 64, D = 64;
const Lay GEN[] = {
    {"encoder_1", 0, 4, 2, 1, 1, 0, 8, 0, 6, G, false, 0, 0, true, false, false, true},
    {"encoder_2", 0, 4, 2, 1, 2, 0, G, 0, G, 2 * G, true, 1, 0},
    {"encoder_3", 0, 4, 2, 1, 4, 0, 2 * G, 0, 2 * G, 2 * G, true, 1, 0},
    {"encoder_4", 0, 4, 2, 1, 8, 0, 2 * G, 0, 2 * G, 4 * G, true, 1, 0},
    {"encoder_fg_1", 0, 4, 2, 1, 1, 0, 8, 0, 3, G, false, 0, 0, true},
    {"merged_encoder_2", 0, 4, 2, 1, 16, 0, 4 * G, 4 * G, 8 * G, 4 * G, true, 1, 0},
    {"merged_encoder_3", 0, 4, 2, 1, 32, 0, 4 * G, 0, 4 * G, 8 * G, true, 1, 0},
    {"merged_encoder_4", 0, 4, 2, 1, 64, 0, 8 * G, 0, 8 * G, 8 * G, true, 1, 0},
    {"merged_encoder_5", 0, 4, 2, 1, 128, 0, 8 * G, 0, 8 * G, 8 * G, true, 1, 0},
    {"merged_decoder_5", 1, 4, 2, 1, 256, 0, 8 * G, 0, 8 * G, 8 * G, true, 2, 0},
    {"merged_decoder_4", 1, 4, 2, 1, 128, 0, 8 * G, 8 * G, 16 * G, 8 * G, true, 2, 0},
    {"merged_decoder_3", 1, 4, 2, 1, 64, 0, 8 * G, 8 * G, 16 * G, 4 * G, true, 2, 0},
    {"merged_decoder_2", 1, 4, 2, 1, 32, 0, 4 * G, 4 * G, 8 * G, 4 * G, true, 2, 0},
    {"merged2_decoder_4", 1, 4, 2, 1, 16, 0, 4 * G, 4 * G, 8 * G, 2 * G, true, 2, 0},
    {"merged2_decoder_3", 1, 4, 2, 1, 8, 0, 2 * G, 2 * G, 4 * G, 2 * G, true, 2, 0},
    {"merged2_decoder_2", 1, 4, 2, 1, 4, 0, 2 * G, 2 * G, 4 * G, G, true, 2, 0},
    {"decoder_1", 1, 4, 2, 1, 2, 0, G, G, 2 * G, 4, false, 2, 0, false, false, true},
};
const Lay DIS[] = {
    {"layer_1", 0, 4, 2, 1, 1, 0, 8, 0, 6, D, false, 0, 0, true},
    {"layer_2", 0, 4, 2, 1, 2, 0, D, 0, D, 2 * D, true, 1, 0},
    {"layer_3", 0, 4, 2, 1, 4, 0, 2 * D, 0, 2 * D, 4 * D, true, 1, 0},
    {"layer_4", 0, 4, 1, 1, 8, 0, 4 * D, 0, 4 * D, 8 * D, true, 1, 0},
    {"layer_5", 0, 4, 1, 1, 8, -1, 8 * D, 0, 8 * D, 1, false, 1, 0, false, false, true},
};
const Lay VGG[] = {
    {"conv1_1", 0, 3, 1, 1, 1, 0, 8, 0, 3, 64, false, 0, 2, true},
    {"conv1_2", 0, 3, 1, 1, 1, 0, 64, 0, 64, 64, false, 0, 2, false, true},
    {"conv2_1", 0, 3, 1, 1, 2, 0, 64, 0, 64, 128, false, 0, 2},
    {"conv2_2", 0, 3, 1, 1, 2, 0, 128, 0, 128, 128, false, 0, 2, false, true},
    {"conv3_1", 0, 3, 1, 1, 4, 0, 128, 0, 128, 256, false, 0, 2},
    {"conv3_2", 0, 3, 1, 1, 4, 0, 256, 0, 256, 256, false, 0, 2, false, true},
    {"conv3_3", 0, 3, 1, 1, 4, 0, 256, 0, 256, 256, false, 0, 2, false, true},
};
const NetDesc NETS[] = {
    {"G", 1, 1, false, false, false, GEN, (int)(sizeof(GEN) / sizeof(GEN[0]))},
    {"D", 3, 3, true, false, true, DIS, (int)(sizeof(DIS) / sizeof(DIS[0]))},
    {"V", 2, 1, true, true, true, VGG, (int)(sizeof(VGG) / sizeof(VGG[0]))},
};

void plan_net(const NetDesc& n, int frames, int side, int bf) {
  const int N = n.mult * frames, alt = n.alt ? frames : 0;
  for (int i = 0; i < n.nl; ++i) {
    const Lay& L = n.l[i];
    const int H = side / L.div + L.off;
    const ConvGeomX g = make_geom(L.kind, L.ks, L.stride, L.pad, N, H, H, L.c0 + L.c1, L.cin_real, L.cout);
    const bool tapgemm = L.kind == 0 && L.stride == 1 && L.ks == 4 && L.cout == 1;
    if (tapgemm) {      // one output channel: the forward as a 1x1 product with 16 rows, float32 out
      const ConvGeomX g1 = make_geom(0, 1, 1, 0, N, H, H, g.Cin, g.Cin, 16);
      IgemmPlan p = plan_fwd(g1, 0, bf);
      p.a.y_f32 = 1;
      plan_kernel(p, 16, bf, g.Cin, 0, 0, LaunchForm{});
      show(n.name, L.name, "fwd", N, bf, p);
    } else {
      IgemmPlan p = plan_fwd(g, 0, bf);
      p.a.ldY = L.f32_out ? g.Cout : g.CoutT; p.a.y_f32 = L.f32_out ? 1 : 0; p.a.out_act = L.out_act;
      LaunchForm f;
      f.bias = !L.bn;
      if (bf && !L.bn && L.out_act == VP_ACT_NONE && !L.f32_out) { f.xa_lrelu = true; f.xa_relu = L.relu_copy; }
      const unsigned fams = (n.groups == 1 && alt == 0 ? FAM_SMALLP : 0) | FAM_PATCH | FAM_PATCH2 | (L.bn && L.out_act == VP_ACT_NONE ? FAM_S2C64 : 0);
      plan_kernel(p, g.Cout, bf, L.c0, L.c1, fams, f);
      show(n.name, L.name, "fwd", N, bf, p);
      if (L.bn) {       // the same launch with batch statistics from its epilogue: shown where it runs another kernel
        LaunchForm fs = p.form;
        fs.stats = true;
        const int ks = pick_conv_kernel(launch_view(p, fs), bf);
        if (ks != p.a.kern) EMIT("%s/%s fwd+stats %d %s: %s", n.name, L.name, N, bf ? "bf16" : "f32", conv_kernel_name(ks));
      }
      if (n.halves && !L.bn) {
        ConvGeomX g2 = g;
        g2.N = alt;
        IgemmPlan h = plan_fwd(g2, 0, bf);
        h.a.ldY = g.CoutT; h.a.out_act = L.out_act;
        LaunchForm fh;
        fh.bias = true;
        plan_kernel(h, g2.Cout, bf, L.c0, L.c1, conv_staging(p.a.kern) == CK_PATCH ? FAM_PATCH : 0, fh, true);
        show(n.name, L.name, "fwd_half", alt, bf, h);
      }
    }
    IgemmPlan bwd[2];
    bool need[2] = {false, false};
    int row0 = 0;
    for (int s = 0; s < (L.c1 ? 2 : 1); ++s) {
      const int rows = s ? L.c1 : L.c0;
      need[s] = !L.from_input || n.input_grads;
      if (need[s]) {
        LaunchForm f;
        f.ref_act = L.in_act != VP_ACT_NONE ? L.in_act : (L.src_relu ? VP_ACT_RELU : VP_ACT_NONE);
        f.ref = !L.from_input && f.ref_act != VP_ACT_NONE;
        bwd[s] = plan_bwd_data(g, 0, row0, rows, L.from_input ? L.cin_real : rows, rows, bf);
        plan_kernel(bwd[s], rows, bf, g.CoutT, 0, (n.groups == 1 && alt == 0 && !L.from_input ? FAM_SMALLP : 0) | FAM_PATCH | FAM_PATCH2, f);
        show(n.name, L.name, s ? "bwd1" : "bwd0", N, bf, bwd[s]);
        if (alt) {
          ConvGeomX g2 = g;
          g2.N = alt;
          IgemmPlan b2 = plan_bwd_data(g2, 0, row0, rows, L.from_input ? L.cin_real : rows, rows, bf);
          plan_kernel(b2, rows, bf, g.CoutT, 0, FAM_PATCH | FAM_PATCH2, f);
          show(n.name, L.name, s ? "bwd1_alt" : "bwd0_alt", alt, bf, b2);
        }
      }
      row0 += rows;
    }
    // the two data gradients of a skip connection as one two-output launch
    if (L.c1 && n.groups == 1 && !alt && need[0] && need[1] && L.c0 == L.c1 && L.cin_real == L.c0 + L.c1 && L.c0 % 32 == 0) {
      const int s0 = conv_staging(bwd[0].a.kern);
      if (s0 == conv_staging(bwd[1].a.kern) && (s0 == CK_IGEMM || s0 == CK_SMALLP)) {
        IgemmPlan p = plan_bwd_data(g, 0, 0, L.c0 + L.c1, L.c0 + L.c1, L.c0, bf);
        p.a.split_c = L.c0;
        LaunchForm f;
        f.ref = true; f.ref_act = L.in_act;
        plan_kernel(p, L.c0 + L.c1, bf, g.CoutT, 0, s0 == CK_SMALLP ? FAM_SMALLP : (L.in_act == VP_ACT_RELU ? FAM_S2C64 : 0), f);
        show(n.name, L.name, "bwd_pair", N, bf, p);
      }
    }
    show_wgrad(n.name, L.name, N, bf, tapgemm ? plan_wgrad(make_geom(0, 1, 1, 0, N, H, H, 16, 16, g.Cin), bf) : plan_wgrad(g, bf));
  }
}

// ---- the single-op entry points (vp_conv_fwd / vp_conv_bwd_data / vp_conv_bwd_weight) on the op-test cases that exist to reach a kernel class ----
struct OpCase { int minblk, kind, n, h, w, cin, cout, k, s, p, in_act, out_act; bool affine; };
const OpCase OPS[] = {
    {384, 0, 8, 256, 256, 32, 128, 4, 2, 1, 0, 0, false},  {384, 0, 8, 96, 96, 256, 512, 4, 1, 1, 0, 0, false},
    {1, 0, 2, 64, 64, 128, 128, 4, 2, 1, 0, 0, false},     {384, 0, 2, 8, 8, 64, 128, 4, 2, 1, 0, 0, false},
    {384, 0, 8, 128, 128, 64, 128, 4, 2, 1, 0, 0, false},  {384, 0, 2, 192, 192, 8, 128, 4, 2, 1, 0, 0, false},
    {384, 1, 8, 64, 64, 256, 64, 4, 2, 1, 0, 0, false},
    {1, 0, 3, 16, 32, 8, 64, 3, 1, 1, 0, 2, false},        {1, 0, 2, 32, 48, 64, 64, 3, 1, 1, 0, 2, false},
    {1, 0, 2, 32, 48, 128, 128, 3, 1, 1, 0, 2, false},     {1, 0, 2, 2, 2, 512, 256, 4, 2, 1, 1, 0, true},
    {1, 0, 5, 4, 4, 256, 128, 4, 2, 1, 1, 0, true},        {1, 1, 2, 8, 8, 128, 4, 4, 2, 1, 2, 3, true},
    {1, 1, 2, 1, 1, 512, 512, 4, 2, 1, 2, 0, true},        {1, 0, 2, 24, 40, 64, 128, 3, 1, 1, 0, 2, false},
    {1, 0, 3, 17, 19, 32, 64, 4, 1, 1, 0, 0, false},       {1, 0, 1, 256, 256, 32, 256, 3, 1, 1, 0, 2, false},
    {1, 0, 2, 256, 256, 32, 128, 3, 1, 1, 0, 2, false},    {1, 0, 4, 256, 256, 64, 256, 4, 2, 1, 0, 0, false},
    {1, 0, 2, 40, 48, 64, 256, 3, 1, 1, 0, 2, false},      {1, 0, 2, 33, 70, 32, 128, 4, 1, 1, 0, 0, false},
    {1, 0, 1, 48, 64, 128, 64, 3, 1, 1, 0, 2, false},      {1, 0, 3, 17, 19, 64, 128, 4, 1, 1, 0, 0, false},
    {1, 1, 2, 8, 8, 128, 64, 4, 2, 1, 0, 0, false},        {1, 0, 4, 64, 128, 8, 64, 3, 1, 1, 0, 2, false},
    {1, 0, 4, 128, 128, 8, 64, 4, 2, 1, 0, 0, false},
};

void plan_ops(int bf) {
  for (const OpCase& c : OPS) {
    vp_tune("patch_min_blocks", c.minblk);
    char name[64];
    snprintf(name, sizeof(name), "k%d_n%d_%dx%d_%dto%d_k%ds%d_mb%d", c.kind, c.n, c.h, c.w, c.cin, c.cout, c.k, c.s, c.minblk);
    const ConvGeomX g = make_geom(c.kind, c.k, c.s, c.p, c.n, c.h, c.w, c.cin, c.cin, c.cout);
    IgemmPlan p = plan_fwd(g, 0, bf);
    p.a.out_act = c.out_act;
    LaunchForm f;
    f.bias = true; f.x_affine = c.affine; f.x_act = c.in_act;
    const bool plain = c.in_act == VP_ACT_NONE && !c.affine;
    plan_kernel(p, g.Cout, bf, c.cin, 0, plain ? (FAM_SMALLP | FAM_PATCH | FAM_PATCH2 | (c.out_act == VP_ACT_NONE ? FAM_S2C64 : 0)) : 0, f);
    show("op", name, "fwd", c.n, bf, p);
    if (c.cout >= 8 && (c.cout & (c.cout - 1)) == 0) {
      IgemmPlan b = plan_bwd_data(g, 0, 0, c.cin, c.cin, c.cin, bf);
      plan_kernel(b, c.cin, bf, c.cout, 0, FAM_SMALLP | FAM_PATCH | FAM_PATCH2, LaunchForm{});
      show("op", name, "bwd", c.n, bf, b);
      show_wgrad("op", name, c.n, bf, plan_wgrad(g, bf, plain));
    }
  }
  vp_tune("patch_min_blocks", -1);
}

// the first sweep prints every line; a later one prints the lines that differ from the first, or only their digest
void sweep(const char* title, bool digest_only = false) {
  static std::vector<std::string> first;
  g_lines.clear();
  static const int plans[3][2] = {{32, 256}, {8, 512}, {4, 256}};      // frames x image side
  for (int bf = 1; bf >= 0; --bf) {
    for (const int(&pl)[2] : plans)
      for (const NetDesc& n : NETS) plan_net(n, pl[0], pl[1], bf);
    plan_ops(bf);
  }
  printf("==== %s ====\n", title);
  if (first.empty()) {
    printf("# net/layer launch images dtype: kernel/family cfg tile splitk CoutPad <IgemmArgs::rowperm, PackDesc::perm, PackDesc::kswap>\n");
    printf("# net/layer wgrad images dtype: cfg tile splitk Mpad Dpad fastw\n");
    for (const std::string& l : g_lines) printf("%s\n", l.c_str());
    first = g_lines;
    return;
  }
  size_t same = 0;
  unsigned long long h = 1469598103934665603ull;      // FNV-1a over the lines that differ
  for (size_t i = 0; i < g_lines.size(); ++i) {
    if (std::find(first.begin(), first.end(), g_lines[i]) != first.end()) { ++same; continue; }      // (every line starts with its plan's name)
    if (!digest_only) printf("%s\n", g_lines[i].c_str());
    for (char c : g_lines[i] + "\n") h = (h ^ (unsigned char)c) * 1099511628211ull;
  }
  if (digest_only) printf("(the others: FNV-1a %016llx)\n", h);
  printf("(%zu of %zu lines as at the default knobs, which have %zu)\n", same, g_lines.size(), first.size());
}

}  // namespace

int main() {
  sweep("default knobs");
  // every kernel-selecting key, one at a time (value to try, value that restores the default)
  static const struct { const char* key; int v, restore; } keys[] = {
      {"c64", 0, 1},   {"dc64", 0, 1},   {"patch3", 0, 1},        {"patch4", 0, 1},      {"patch2", 0, 1},      {"s2c64", 0, 512},
      {"smallp_max_pixels", 0, 256},     {"patch_tiles", 1, 7},   {"patch_tiles", 2, 7}, {"patch_tiles", 4, 7}, {"patch_min_blocks", 1, -1},
  };
  for (const auto& k : keys) {
    char title[64];
    snprintf(title, sizeof(title), "%s=%d", k.key, k.v);
    vp_tune(k.key, k.v);
    sweep(title);
    vp_tune(k.key, k.restore);
  }
  sweep("default knobs again");
  // vp_tune's return codes, and that a refused or reset value leaves the plans as they were
  static const char* const all[] = {"patch_tiles", "patch_min_blocks", "patch_small_tiles", "patch_long_k_on_256", "wgrad_tr", "patch3", "c64", "dc64",
                                    "pool_bwd_fused", "cout1_wgrad_rows", "cout1_bwd", "s2c64", "wgrad_big", "patch4", "s2c64_pair", "bfm_dwproj", "patch2",
                                    "patch_xcd", "smallp_max_pixels", "igemm_splitk_target", "wgrad_fixed_x10", "wgrad_slab_tile_x1000", "wgrad_slab_x100",
                                    "smallp_split_target", "igemm_splitk_cap", "igemm_splitk_minchunk", "wgrad_resident_blocks", "igemm_small_grid",
                                    "thin_blocks_cout8", "thin_blocks_dcout8", "thin_blocks_cout4", "thin_blocks_cin8", "phase_marks", "no_such_key"};
  printf("==== vp_tune return codes ====\n");
  for (const char* key : all) {
    printf("%s:", key);
    for (int v : {-1, 0, 5}) printf(" %d->%d", v, vp_tune(key, v));
    printf("\n");
  }
  printf("null key -> %d\n", vp_tune(nullptr, 1));
  // what every knob holds after -1, 0, 5 in that order shows in the plans: as a digest of the lines that moved
  sweep("after the return-code pass", true);
  return 0;
}
