"""Every plan-time choice of the convolution launch path, without a GPU: tests/conv_choice.cpp plans the PixReferNet generator,
discriminator and VGG layers at the three BASELINE plans (32 x 256^2, 8 x 512^2, 4 x 256^2) and the op-test cases that exist to reach a
kernel class, in bf16 and f32, at the default knobs and under every kernel-selecting vp_tune key, and prints kernel, family, tile, K
split and packed-weight layout of each plan, the weight-gradient plans, and vp_tune's return codes (a sweep after the first prints the
lines that moved).  Its output must equal
tests/golden/conv_choice.txt, recorded from the library before the kernel table (conv_dispatch.hip) replaced the hand-kept switches.

When a later change moves a heuristic on purpose, regenerate the golden from the new library and review its diff line by line:
  make -C voicepuppet_amd/csrc host-asan
  clang++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM/include -Iinclude -Ivoicepuppet_amd/csrc tests/conv_choice.cpp \\
      -Lvoicepuppet_amd -l:libvp_host_asan.so -Wl,-rpath,$PWD/voicepuppet_amd -Wl,-rpath,$ROCM/lib -o /tmp/conv_choice
  /tmp/conv_choice > tests/golden/conv_choice.txt
"""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voicepuppet_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_choice.txt")
KERNELS = ("igemm", "patch", "patch2", "smallp", "s2c64", "cin8", "cout8", "dcout8", "cout4", "c64", "patch3", "patch4", "dc256", "dc64")


def test_golden_reaches_every_kernel_at_default_knobs():
  text = open(GOLDEN).read()
  default = text.split("==== c64=0 ====")[0]
  assert default.startswith("==== default knobs ====\n")
  for k in KERNELS:
    assert ": %s/" % k in default, k
  for dtype in ("bf16", "f32"):
    assert " fwd 32 %s: " % dtype in default and " wgrad 32 %s: " % dtype in default
  assert "==== default knobs again ====\n(875 of 875 lines as at the default knobs, which have 875)\n" in text      # every key restored
  assert "no_such_key: -1->-1 0->-1 5->-1\n" in text


def test_choices_equal_the_recorded_library_under_sanitizers():
  """The stand-alone program against the `make host-asan` build of the host layer (AddressSanitizer + UBSan, kernels reduced to launch
  stubs; no Python in the process): byte-for-byte the golden, the sanitizers silent."""
  hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  clang = "/opt/rocm/lib/llvm/bin/clang++"
  if not (os.path.exists(hipcc) and os.path.exists(clang)):
    pytest.skip("no hipcc: the sanitizer build needs the HIP host compiler")
  b = subprocess.run(["make", "-C", CSRC, "-j4", "host-asan"], capture_output=True, text=True, timeout=900)
  assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
  libdir = os.path.join(ROOT, "voicepuppet_amd")
  with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "conv_choice")
    c = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                        "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "conv_choice.cpp"),
                        "-L", libdir, "-l:libvp_host_asan.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stdout[-2000:] + c.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
  want = open(GOLDEN).read()
  if r.stdout != want:
    got, exp = r.stdout.split("\n"), want.split("\n")
    first = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    pytest.fail("line %d differs (%d lines, golden %d):\n  got  %s\n  want %s" % (first + 1, len(got), len(exp), got[first:first + 1], exp[first:first + 1]))
