"""Build every native artefact in-tree (no JIT cache, no pip install).

  libmobiclip_hip.so      product: host parser + C ABI + gfx950 kernels          (hipcc)
  libmobiclip_hip_prof.so the same sources with -DMOBI_PROFILING (debug hooks, ablation switches): tools/ and two tests only
  libmobi_streamgen.so    synthetic bitstream generator (input source)           (g++)
  oracle/_build/libmobi_oracle.so   CPU oracle = TEST INFRASTRUCTURE             (gcc)
  tests/tools/libmobi_cmdinterp.so  CPU command-list interpreter = TEST TOOL     (g++)
  tests/tools/libmobi_lsparse_host.so  lock-step parser's lane functions on the CPU = TEST TOOL (g++)
  tests/tools/libmobi_idle_host.so  the frame-parallel chain's kernel bodies on the CPU, idle slots = TEST TOOL (g++)
  tests/tools/libmobi_audio_host.so  the audio arithmetic header (csrc/mobi_audio.h) on the CPU = TEST TOOL (g++)
  tests/tools/libmobi_sx_host.so  the Sx arithmetic header (csrc/mobi_sx.h) on the CPU = TEST TOOL (g++)
  tests/tools/libmobi_motionhost.so  "command list -> motion" (csrc/mobi_motion.h) on the CPU = TEST TOOL (g++)
  tests/tools/libmobi_encode_host.so  the intra encoder (csrc/mobi_encode.h) on the CPU: the host model = TEST TOOL (g++)
  tests/tools/libmobi_encode_inter_host.so  the inter encoder (csrc/mobi_encode_inter.h) on the CPU: the host model = TEST TOOL (g++)
  tests/tools/libmobi_encode_parts_host.so  the inter encoder with partitions (csrc/mobi_encode_parts.h) on the CPU: the host model = TEST TOOL (g++)
  tests/tools/libmobi_encode_pintra_host.so  the inter encoder with its intra mode (csrc/mobi_encode_pintra.h) on the CPU: the host model = TEST TOOL (g++)
  tests/tools/libmobi_encode_rate_host.so  the rate rule (csrc/mobi_encode_rate.h) over those three models' picture functions on the CPU = TEST TOOL (g++)
      (the first three by build_enc_host, over tests/tools/enc_host_pool.h; the encoders' shared host side, csrc/mobi_encode_ctx.h, is part of the product)
  tests/tools/libmobi_mux_host.so  the muxing rule (csrc/mobi_mux.h) on the CPU: begin, append, finish = TEST TOOL (g++)
  tests/tools/libmobi_mux_audio_host.so  the muxing rule with an audio stream (csrc/mobi_mux.h, include/mobiclip_mux_audio.h) on the CPU = TEST TOOL (g++)
  tests/tools/libmobi_audio_enc_host.so  the audio encoder's rule (csrc/mobi_audio_enc.h) on the CPU = TEST TOOL (g++)
  tests/tools/abi_caller            plain-C caller of the product's C ABI = TEST TOOL (gcc)

hipcc cross-compiles gfx950 without a GPU.  The built .so files are git-ignored but travel to the
GPU box with the gpurun snapshot.
"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mobiclipdecoder_amd")
CSRC = os.path.join(PKG, "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")

LIB_HIP = os.path.join(PKG, "libmobiclip_hip.so")
LIB_HIP_PROF = os.path.join(PKG, "libmobiclip_hip_prof.so")  # -DMOBI_PROFILING twin: tools/ and the tests that inject planes
LIB_GEN = os.path.join(PKG, "libmobi_streamgen.so")
LIB_ORACLE = os.path.join(ROOT, "oracle", "_build", "libmobi_oracle.so")
LIB_INTERP = os.path.join(ROOT, "tests", "tools", "libmobi_cmdinterp.so")
LIB_LSHOST = os.path.join(ROOT, "tests", "tools", "libmobi_lsparse_host.so")  # the lock-step parser's lane functions on the CPU (test tool)
LIB_IDLEHOST = os.path.join(ROOT, "tests", "tools", "libmobi_idle_host.so")  # mobi_gop_prepare / mobi_gop_chain bodies on the CPU (test tool)
LIB_AUDIOHOST = os.path.join(ROOT, "tests", "tools", "libmobi_audio_host.so")  # csrc/mobi_audio.h's per-sample arithmetic on the CPU (test tool)
LIB_SXHOST = os.path.join(ROOT, "tests", "tools", "libmobi_sx_host.so")  # csrc/mobi_sx.h's packet arithmetic on the CPU (test tool)
LIB_MOTIONHOST = os.path.join(ROOT, "tests", "tools", "libmobi_motionhost.so")  # csrc/mobi_motion.h's reading of a command list on the CPU (test tool)
LIB_ENCHOST = os.path.join(ROOT, "tests", "tools", "libmobi_encode_host.so")  # csrc/mobi_encode.h's whole encoder on the CPU (test tool)
LIB_ENCINTERHOST = os.path.join(ROOT, "tests", "tools", "libmobi_encode_inter_host.so")  # csrc/mobi_encode_inter.h's whole encoder on the CPU (test tool)
LIB_ENCPARTSHOST = os.path.join(ROOT, "tests", "tools", "libmobi_encode_parts_host.so")  # csrc/mobi_encode_parts.h's whole encoder on the CPU (test tool)
LIB_ENCPINTRAHOST = os.path.join(ROOT, "tests", "tools", "libmobi_encode_pintra_host.so")  # csrc/mobi_encode_pintra.h's whole encoder on the CPU (test tool)
LIB_ENCRATEHOST = os.path.join(ROOT, "tests", "tools", "libmobi_encode_rate_host.so")  # csrc/mobi_encode_rate.h's bisection over the three models (test tool)
LIB_MUXHOST = os.path.join(ROOT, "tests", "tools", "libmobi_mux_host.so")  # csrc/mobi_mux.h's begin, append and finish on the CPU (test tool)
LIB_MUXAUDIOHOST = os.path.join(ROOT, "tests", "tools", "libmobi_mux_audio_host.so")  # csrc/mobi_mux.h's sessions of video and audio frames on the CPU (test tool)
LIB_AUDIOENCHOST = os.path.join(ROOT, "tests", "tools", "libmobi_audio_enc_host.so")  # csrc/mobi_audio_enc.h's whole encoder on the CPU (test tool)
ABI_CALLER = os.path.join(ROOT, "tests", "tools", "abi_caller")  # plain-C caller of the product library (test tool)


# the sources of libmobiclip_hip.so: *.cpp are host objects (g++), *.hip kernel objects (hipcc --offload-arch=gfx950); linked in this order
HIP_SOURCES = ("mobi_batch.cpp", "mobi_step_host.cpp", "mobi_step_device.cpp", "mobi_step_groups.cpp", "mobi_replay.cpp", "mobi_pictures.cpp", "mobi_parse.cpp", "mobi_demux.cpp", "mobi_moflex.cpp", "mobi_export.cpp", "mobi_txcode.cpp", "mobi_audio_plan.cpp", "mobi_audio.cpp", "mobi_kernels.hip", "mobi_rgb.hip", "mobi_dparse.hip", "mobi_lsparse.hip", "mobi_gop.hip", "mobi_analysis.hip", "mobi_export.hip", "mobi_txcode.hip", "mobi_export_rgb.hip", "mobi_export_scale.hip", "mobi_export_resample.hip", "mobi_reset.hip", "mobi_idle.hip", "mobi_audio.hip", "mobi_sx.hip", "mobi_motion.hip", "mobi_sink.cpp", "mobi_sink.hip", "mobi_encode.cpp", "mobi_encode.hip", "mobi_encode_inter.cpp", "mobi_encode_inter.hip", "mobi_encode_parts.hip", "mobi_encode_pintra.hip", "mobi_encode_rate.hip", "mobi_mux.cpp", "mobi_mux.hip", "mobi_mux_audio.hip", "mobi_audio_enc.cpp", "mobi_audio_enc.hip")


def hip_objects(profiling=False):
    """the object files build_hip links, in link order (python -m mobiclipdecoder_amd.build --objects [--profiling]: tools/ that rebuild one of them)"""
    obj = os.path.join(PKG, "_obj_prof" if profiling else "_obj")
    return [os.path.join(obj, f + ".o") for f in HIP_SOURCES]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _hdrs(d):
    return [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".h")]


def header_symbols():
    """every function include/*.h declares (the C ABI)"""
    import re
    names = []
    for h in ("mobiclip_hip.h", "mobiclip_demux.h", "mobiclip_audio.h", "mobiclip_sx.h", "mobiclip_encode.h", "mobiclip_encode_inter.h", "mobiclip_encode_parts.h", "mobiclip_encode_pintra.h", "mobiclip_encode_rate.h", "mobiclip_mux.h", "mobiclip_mux_audio.h", "mobiclip_audio_enc.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        names += re.findall(r"\b(mobi_\w+)\s*\(", text)
    return sorted(set(names))


def build_hip(force=False, profiling=False):
    """profiling=True (python -m mobiclipdecoder_amd.build --profiling, tools/ only): a SECOND library, libmobiclip_hip_prof.so, with
    -DMOBI_PROFILING: the ablation / occupancy / stage-stop switches (MOBI_INTRA_DBG, MOBI_LDS_PAD, MOBI_INTRA_LDS_PAD, MOBI_STOP_STAGE,
    MOBI_DEBUG=9) and the mobi_debug_* test hooks.  The product library has none of them; tools select the other one with MOBI_LIB."""
    srcs = [os.path.join(CSRC, f) for f in HIP_SOURCES]
    deps = srcs + _hdrs(CSRC) + [os.path.join(ROOT, "include", "mobiclip_hip.h"), os.path.join(ROOT, "include", "mobiclip_demux.h"), os.path.join(ROOT, "include", "mobiclip_audio.h"),
                                  os.path.join(ROOT, "include", "mobiclip_sx.h"), os.path.join(ROOT, "include", "mobiclip_encode.h"), os.path.join(ROOT, "include", "mobiclip_encode_inter.h"), os.path.join(ROOT, "include", "mobiclip_encode_parts.h"), os.path.join(ROOT, "include", "mobiclip_encode_pintra.h"), os.path.join(ROOT, "include", "mobiclip_encode_rate.h"), os.path.join(ROOT, "include", "mobiclip_mux.h"), os.path.join(ROOT, "include", "mobiclip_mux_audio.h"), os.path.join(ROOT, "include", "mobiclip_audio_enc.h"), os.path.abspath(__file__)]
    lib = LIB_HIP_PROF if profiling else LIB_HIP
    if not force and not _newer(lib, deps):
        return lib
    obj = os.path.join(PKG, "_obj_prof" if profiling else "_obj")
    os.makedirs(obj, exist_ok=True)
    prof = ["-DMOBI_PROFILING"] if profiling else []
    # only the entry points include/*.h declare leave the library (MOBI_API); everything else is hidden
    # (-O3: the host parser -- hand-overs, small batches, mobi_decode -- parses a 640x480 P-frame in 0.41 ms instead of 0.47)
    host_flags = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-fwrapv", "-fvisibility=hidden", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")] + prof
    objs = hip_objects(profiling)
    for s, o in zip(srcs, objs):
        if s.endswith(".cpp"):
            _run(["g++"] + host_flags + ["-c", s, "-o", o])
    # the reconstruction kernels are bound by instruction issue: LLVM's ILP-first scheduling is worth 1.5 % on mobi_recon_inter8
    # (same registers, same occupancy; measured A/B on one box); the other kernels keep the default
    # r03: both kernels are bound by vector instruction issue; loops the source does not ask to unroll stay loops (-fno-unroll-loops:
    # 2.51 against 2.57 ms per launch of 8192 clips, tools/exp_kernel_flags.sh)
    extra = {"mobi_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fno-unroll-loops"],
             # the lock-step parser is one long dependent chain per wave: 24.8 against 25.6 ms per P-frame step (tools/exp_lsflags.sh)
             "mobi_lsparse.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]}
    for s, ko in zip(srcs, objs):
        if s.endswith(".hip"):
            _run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"] + prof + extra.get(os.path.basename(s), []) + ["-c", s, "-o", ko])
    # What leaves the library is exactly what include/*.h declares (the profiling twin adds its mobi_debug_* hooks): a linker version
    # script written from the headers -- no C++ symbols, no template instantiations, no kernel stubs.
    vs = os.path.join(obj, "exports.map")
    with open(vs, "w") as f:
        f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in header_symbols()) + ("    mobi_debug_*;\n" if profiling else "") + "  local: *;\n};\n")
    _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + vs] + objs + ["-o", lib])
    return lib


def build_gen(force=False):
    src = os.path.join(CSRC, "mobi_streamgen.cpp")
    if force or _newer(LIB_GEN, [src] + _hdrs(CSRC)):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", src, "-o", LIB_GEN])
    return LIB_GEN


def build_oracle(force=False):
    odir = os.path.join(ROOT, "oracle")
    src = os.path.join(odir, "mobi_oracle.c")
    if force or _newer(LIB_ORACLE, [src] + _hdrs(odir)):
        os.makedirs(os.path.dirname(LIB_ORACLE), exist_ok=True)
        _run(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off", "-Wall", src, "-o", LIB_ORACLE])
    return LIB_ORACLE


def build_interp(force=False):
    src = os.path.join(ROOT, "tests", "tools", "mobi_cmd_interp.cpp")
    parse = os.path.join(CSRC, "mobi_parse.cpp")
    if force or _newer(LIB_INTERP, [src, parse] + _hdrs(CSRC)):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-fwrapv", src, parse, "-o", LIB_INTERP])
    return LIB_INTERP


def build_lshost(force=False):
    src = os.path.join(ROOT, "tests", "tools", "mobi_lsparse_host.cpp")
    parse = os.path.join(CSRC, "mobi_parse.cpp")
    if force or _newer(LIB_LSHOST, [src, parse] + _hdrs(CSRC)):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-fwrapv", "-I" + CSRC, src, parse, "-o", LIB_LSHOST])
    return LIB_LSHOST


def build_idlehost(force=False):
    src = os.path.join(ROOT, "tests", "tools", "mobi_idle_host.cpp")
    parse = os.path.join(CSRC, "mobi_parse.cpp")
    if force or _newer(LIB_IDLEHOST, [src, parse] + _hdrs(CSRC)):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-fwrapv", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC, src, parse, "-o", LIB_IDLEHOST])
    return LIB_IDLEHOST


def build_audiohost(force=False):
    src = os.path.join(ROOT, "tests", "tools", "mobi_audio_host.cpp")
    if force or _newer(LIB_AUDIOHOST, [src, os.path.join(CSRC, "mobi_audio.h"), os.path.join(ROOT, "include", "mobiclip_audio.h")]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + CSRC, src, "-o", LIB_AUDIOHOST])
    return LIB_AUDIOHOST


def build_sxhost(force=False):
    src = os.path.join(ROOT, "tests", "tools", "mobi_sx_host.cpp")
    plan = os.path.join(CSRC, "mobi_audio_plan.cpp")
    hdrs = [os.path.join(CSRC, "mobi_sx.h"), os.path.join(CSRC, "mobi_audio.h"), os.path.join(ROOT, "include", "mobiclip_sx.h"), os.path.join(ROOT, "include", "mobiclip_audio.h")]
    if force or _newer(LIB_SXHOST, [src, plan] + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + CSRC, src, plan, "-o", LIB_SXHOST])
    return LIB_SXHOST


def build_motionhost(force=False):
    src = os.path.join(ROOT, "tests", "tools", "mobi_motion_host.cpp")
    if force or _newer(LIB_MOTIONHOST, [src] + [os.path.join(CSRC, h) for h in ("mobi_motion.h", "mobi_syntax.h", "mobi_cmd.h")]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-fwrapv", "-I" + CSRC, src, "-o", LIB_MOTIONHOST])
    return LIB_MOTIONHOST


def build_enc_host(inter, force=False, parts=False):
    """the host model of the intra (inter=False) or the inter encoder, or of the inter encoder with partitions (parts=True):
    tests/tools/mobi_encode[_inter|_parts]_host.cpp over the headers beside it (tests/tools/enc_host_pool.h; whichever are there: the
    sources under tests/ say what they include, this list only what to watch)"""
    lib, name = (LIB_ENCPARTSHOST, "mobi_encode_parts") if parts else (LIB_ENCINTERHOST, "mobi_encode_inter") if inter else (LIB_ENCHOST, "mobi_encode")
    src = os.path.join(ROOT, "tests", "tools", name + "_host.cpp")
    first = 0 if parts else 1 if inter else 2
    hdrs = [os.path.join(CSRC, h) for h in ("mobi_encode_parts.h", "mobi_encode_inter.h", "mobi_encode.h", "mobi_txcode.h", "mobi_recon_math.h", "mobi_tables.h")[first:]]
    hdrs += [os.path.join(ROOT, "include", h) for h in ("mobiclip_encode_parts.h", "mobiclip_encode_inter.h", "mobiclip_encode.h")[first:]] + _hdrs(os.path.join(ROOT, "tests", "tools"))
    if force or _newer(lib, [src] + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-I" + CSRC, src, "-o", lib])
    return lib


def build_enchost(force=False):
    return build_enc_host(False, force)


def build_encinterhost(force=False):
    return build_enc_host(True, force)


def build_encpartshost(force=False):
    return build_enc_host(True, force, parts=True)


def build_encpintrahost(force=False):
    """the host model of the inter encoder's intra mode: tests/tools/mobi_encode_pintra_host.cpp over csrc/mobi_encode_pintra.h and the two encoders' headers"""
    src = os.path.join(ROOT, "tests", "tools", "mobi_encode_pintra_host.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("mobi_encode_pintra.h", "mobi_encode_inter.h", "mobi_encode.h", "mobi_txcode.h", "mobi_recon_math.h", "mobi_tables.h")]
    hdrs += [os.path.join(ROOT, "include", h) for h in ("mobiclip_encode_pintra.h", "mobiclip_encode_inter.h", "mobiclip_encode.h")] + _hdrs(os.path.join(ROOT, "tests", "tools"))
    if force or _newer(LIB_ENCPINTRAHOST, [src] + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-I" + CSRC, src, "-o", LIB_ENCPINTRAHOST])
    return LIB_ENCPINTRAHOST


def build_encratehost(force=False):
    """the host model of the rate rule: tests/tools/mobi_encode_rate_host.cpp over csrc/mobi_encode_rate.h and the three encoders' headers"""
    src = os.path.join(ROOT, "tests", "tools", "mobi_encode_rate_host.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("mobi_encode_rate.h", "mobi_encode_parts.h", "mobi_encode_inter.h", "mobi_encode.h", "mobi_txcode.h", "mobi_recon_math.h", "mobi_tables.h")]
    hdrs += [os.path.join(ROOT, "include", h) for h in ("mobiclip_encode_rate.h", "mobiclip_encode_parts.h", "mobiclip_encode_inter.h", "mobiclip_encode.h")] + _hdrs(os.path.join(ROOT, "tests", "tools"))
    if force or _newer(LIB_ENCRATEHOST, [src] + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-variable", "-fwrapv", "-pthread", "-I" + CSRC, src, "-o", LIB_ENCRATEHOST])
    return LIB_ENCRATEHOST


def build_muxhost(force=False):
    """the host model of the muxer: tests/tools/mobi_mux_host.cpp over csrc/mobi_mux.h"""
    src = os.path.join(ROOT, "tests", "tools", "mobi_mux_host.cpp")
    if force or _newer(LIB_MUXHOST, [src, os.path.join(CSRC, "mobi_mux.h"), os.path.join(ROOT, "include", "mobiclip_mux.h"), os.path.join(ROOT, "include", "mobiclip_mux_audio.h"), os.path.join(ROOT, "include", "mobiclip_hip.h")]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + CSRC, src, "-o", LIB_MUXHOST])
    return LIB_MUXHOST


def build_muxaudiohost(force=False):
    """the host model of the muxer with an audio stream: tests/tools/mobi_mux_audio_host.cpp over csrc/mobi_mux.h"""
    src = os.path.join(ROOT, "tests", "tools", "mobi_mux_audio_host.cpp")
    if force or _newer(LIB_MUXAUDIOHOST, [src, os.path.join(CSRC, "mobi_mux.h")] + [os.path.join(ROOT, "include", h) for h in ("mobiclip_mux.h", "mobiclip_mux_audio.h", "mobiclip_hip.h")]):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + CSRC, src, "-o", LIB_MUXAUDIOHOST])
    return LIB_MUXAUDIOHOST


def build_audioenchost(force=False):
    """the host model of the audio encoder: tests/tools/mobi_audio_enc_host.cpp over csrc/mobi_audio_enc.h"""
    src = os.path.join(ROOT, "tests", "tools", "mobi_audio_enc_host.cpp")
    hdrs = [os.path.join(CSRC, "mobi_audio_enc.h"), os.path.join(CSRC, "mobi_audio.h")] + [os.path.join(ROOT, "include", h) for h in ("mobiclip_audio_enc.h", "mobiclip_audio.h", "mobiclip_hip.h")]
    if force or _newer(LIB_AUDIOENCHOST, [src] + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread", "-I" + CSRC, src, "-o", LIB_AUDIOENCHOST])
    return LIB_AUDIOENCHOST


def build_caller(force=False):
    src = os.path.join(ROOT, "tests", "tools", "abi_caller.c")
    if force or _newer(ABI_CALLER, [src, os.path.join(ROOT, "include", "mobiclip_hip.h"), LIB_HIP]):
        _run(["gcc", "-O2", "-std=c99", "-Wall", src, "-L" + PKG, "-lmobiclip_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath-link," + os.path.join(ROCM, "lib"), "-o", ABI_CALLER])
    return ABI_CALLER


def build_all(force=False):
    return [build_hip(force), build_hip(force, profiling=True), build_gen(force), build_oracle(force), build_interp(force), build_lshost(force), build_idlehost(force), build_audiohost(force), build_sxhost(force), build_motionhost(force), build_enchost(force), build_encinterhost(force), build_encpartshost(force), build_encpintrahost(force), build_encratehost(force), build_muxhost(force), build_muxaudiohost(force), build_audioenchost(force), build_caller(force)]


if __name__ == "__main__":
    if "--objects" in sys.argv:
        print(" ".join(hip_objects("--profiling" in sys.argv)))
        sys.exit(0)
    if "--profiling" in sys.argv:
        build_hip(force="--force" in sys.argv, profiling=True)
    else:
        build_all(force="--force" in sys.argv)
    print("ok")
