"""The per-env LDS carve (csrc/vmp_carve.h) on the CPU, under ASan + UBSan:
tests/native/carve_sweep.cpp sweeps 132 649 (P, V, kernel) configs for the
carve's invariants (alignment, bounds, disjoint regions per phase), compares
the carve fields with tests/golden/carve_fields.csv (44 configs field by field,
the whole grid by hash and by the count of configs that fit), and checks that
the launch, fit-check and occupancy sizes agree. No library, no device.

The fixture is the output of `carve_sweep --emit` with the carve functions of
vmp_capi.cpp as they stood before vmp_carve.h replaced them (carve(),
carve_big(), big_shape() and vmp_create's fit check, verbatim, in a throwaway
driver): the carve must stay what it was.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vm-placement-migration-gym_amd")


def test_carve_sweep_under_asan_ubsan():
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
             UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run(["make", "-s", "-C", PKG, "carve-sweep"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    p = subprocess.run([os.path.join(PKG, "build", "san", "carve_sweep"),
                        os.path.join(ROOT, "tests", "golden", "carve_fields.csv")],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert "132649 configs, 116581 fit, 0 violations" in out, out[-4000:]
    assert "carve sweep ok" in out
