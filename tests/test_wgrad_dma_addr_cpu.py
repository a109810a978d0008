"""The LDS-DMA address arithmetic of the all-taps weight-gradient kernels (csrc/wgrad_dma_addr.inc: conv_wgrad_c128b.hip and
conv_wgrad_s2.hip include it) against a literal restatement of the arithmetic the kernels carried in their tile loops before,
on the host: tests/wgrad_dma_addr_check.cpp is built with the host compiler and walks every (tile, wave, slot, lane) of the
geometries of tests/test_wgrad_dma_addr_gpu.py and of the five benchmark layers.  A wrong source address is a GPU fault, so
this runs where no GPU is needed."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler (CXX, c++, g++, clang++) to build tests/wgrad_dma_addr_check.cpp with")


def test_new_addresses_equal_the_former_ones_and_stay_in_bounds(tmp_path):
    exe = str(tmp_path / "wgrad_dma_addr_check")
    src = os.path.join(HERE, "wgrad_dma_addr_check.cpp")
    assert os.path.exists(os.path.join(ROOT, "multimodal-isic_amd", "csrc", "wgrad_dma_addr.inc"))
    b = subprocess.run([_host_compiler(), "-O1", "-std=c++17", "-Wall", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(", 0 failures") and int(last.split()[0]) > 4_000_000, last
