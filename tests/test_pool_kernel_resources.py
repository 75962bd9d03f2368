"""What the headline's pool kernel may cost (no GPU needed): the baked `c2` instance of raytracingpbr_amd/prebuild.py —
the code object bench.py's flagship step runs — is compiled (or found in the catalog build() fills) and the resource
notes of its code object are read.  rt_jit_trace is compiled for six waves per SIMD and seven blocks per CU:
  * at most 80 VGPRs (512 / 6 = 85, allocated in eights),
  * no scratch: a spill in the march loop or around a shading pass is memory traffic per step (rt_trace.hpp, RT_POOL_WAVES),
  * at most 23 405 bytes of LDS: 160 KB / 7 blocks.
"""
import os
import re
import subprocess

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def kernel_notes(path, tmp_path):
    obj = str(tmp_path / "k.o")
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + path, "--output=" + obj], check=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], capture_output=True, text=True, check=True).stdout
    out = {}
    # one "- .args: ... .name: X ... .wavefront_size: 64" mapping per kernel; scalar entries are "    .key:   value"
    for chunk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        kv = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", chunk, re.M))
        out[kv[".name"]] = kv
    return out


def test_baked_headline_pool_kernel_fits_six_waves_and_seven_blocks(tmp_path):
    from raytracingpbr_amd import prebuild
    entry = [e for e in prebuild.DEFAULT if e[0] == "c2"]
    assert entry and entry[0][4] == "jit=1 jit_bake=2"
    path = prebuild.prebuild(entry)["c2"]
    k = kernel_notes(path, tmp_path)["rt_jit_trace"]
    print("rt_jit_trace:", {key: k[key] for key in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")})
    assert int(k[".vgpr_count"]) <= 80
    assert int(k[".private_segment_fixed_size"]) == 0 and int(k[".vgpr_spill_count"]) == 0
    assert int(k[".group_segment_fixed_size"]) <= 23405
