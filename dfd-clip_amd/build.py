"""Builds libdfdclip_hip.so (hand-written gfx950 kernels + C ABI) in-tree with hipcc.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU, so the build runs in the CPU
container and the resulting .so travels to the GPU box with the source snapshot.
"""
import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
OBJ_DIR = os.path.join(CSRC, "build")
LIB_PATH = os.path.join(PKG_DIR, "libdfdclip_hip.so")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include")
ARCH = "gfx950"
FLAGS = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function"]
# Kernels whose hand-counted `s_waitcnt vmcnt(N)` are exact only while the compiler adds no vector-memory operation of
# its own: a register spill (scratch_store / scratch_load counts in vmcnt) would silently turn a wait into a race.  The
# build asks the compiler for its resource report on these files and refuses a kernel with scratch.
# (Every form of gemm256e.hip, bf16 and fp8, is held to this: its loop never waits for zero.  gemm256p.hip's fp8 forms
# spill 2 to 8 registers (8 to 32 bytes per lane); its K loop waits for vmcnt(0) every step, so that only over-waits
# there, and it is not in the list.  Both kernels inline one epilogue, tile_epilogue in gemm256p_common.hpp.)
# align.hip has no hand-counted waits; it is listed because a spill in its tap loop would put scratch traffic on a kernel
# whose whole cost is memory operations.  elastic.hip's remap kernel is listed for the same reason: it holds sixteen tap
# offsets and weights per lane across its frame loop (both instantiations are checked).  yuv.hip's two kernels (both names
# hold "yuv420_") are byte movers as well: the converter keeps six 8-byte results per lane, the fused gather align.hip's state.
# swiglu.hip's gate kernels (every instantiation holds "swiglu_") move three elements per result and nothing else.
# kv_gather.hip's row gathers ("kv_gather_": both forms, every instantiation) move two rows per lane and nothing else.
# kv_frames.hip's frame movers ("kv_frames_": both forms, both load policies) move two rows per lane through two tables.
# adapter.hip's kernels ("adapter_") are HBM-bound and the register-resident backward sits at the 128-VGPR ceiling of its 1024 threads.
# optim.hip's EMA blend ("ema_step_kernel", both stream-policy forms) moves two loads and one or two stores per element.
NO_SCRATCH = {"optim.hip": "ema_step_kernel", "gemm256e.hip": "gemm256e_kernel", "attention_mfma_xrow.hip": "attn_mfma_xrow_kernel", "align.hip": "align_crop_u8_kernel",
              "elastic.hip": "elastic_remap_u8_kernel", "yuv.hip": "yuv420_", "swiglu.hip": "swiglu_", "kv_gather.hip": "kv_gather_",
              "kv_frames.hip": "kv_frames_",
              "adapter.hip": "adapter_"}


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP kernels cannot be built")
    return exe


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _digest(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def scratch_users(report, kernel_substr):
    """From hipcc's -Rpass-analysis=kernel-resource-usage remarks: {kernel: bytes/lane} for kernels using scratch."""
    import re
    out, name = {}, None
    for line in report.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and kernel_substr in name and int(m.group(1)) > 0:
            out[name] = int(m.group(1))
    return out


def build(force=False, verbose=False, extra_flags=()):
    """Compile every .hip under csrc/ and link the shared library.  Returns its path.
    Incremental: an object is rebuilt when its source, a header or the flags changed."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hpp")]
    headers.append(os.path.join(INCLUDE, "dfdclip.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_ext.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_explain.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_augment.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_align.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_elastic.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_yuv.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_swiglu.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_kvgather.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_kvframes.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_kvtable.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_ema.h"))
    headers.append(os.path.join(INCLUDE, "dfdclip_hooks.h"))
    jobs, objs = [], []
    for src in sources():
        sp = os.path.join(CSRC, src)
        obj = os.path.join(OBJ_DIR, src[:-4] + ".o")
        stamp = obj + ".sha"
        dig = _digest([sp] + headers) + " ".join(extra_flags)
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig:
            continue
        jobs.append((sp, obj, stamp, dig))

    def compile_one(job):
        sp, obj, stamp, dig = job
        guard = NO_SCRATCH.get(os.path.basename(sp))
        cmd = [hipcc, *FLAGS, *extra_flags, *(["-Rpass-analysis=kernel-resource-usage"] if guard else []), "-c", sp, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {sp}:\n{r.stderr}")
        if guard:
            bad = scratch_users(r.stderr, guard)
            if bad:
                raise RuntimeError(f"{sp}: kernels listed in NO_SCRATCH must not use scratch, but: {bad}")
        elif verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        with open(stamp, "w") as f:
            f.write(dig)
        return sp

    if jobs:
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            for done in ex.map(compile_one, jobs):
                if verbose:
                    print("built", os.path.basename(done))
    if jobs or not os.path.exists(LIB_PATH):
        r = subprocess.run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB_PATH, *objs],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
