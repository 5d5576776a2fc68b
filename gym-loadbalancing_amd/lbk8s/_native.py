"""ctypes binding of liblbk8s.so (include/lbk8s.h).

The library is built in-tree (gym-loadbalancing_amd/csrc/Makefile) next to this file.
torch is imported BEFORE the library is loaded so that liblbk8s.so's dependency on
libamdhip64.so.7 resolves (by soname) to the HIP runtime torch already loaded: one HIP
runtime per process, so torch's streams and allocations are valid in our calls.
There is no CPU fallback: if the library is missing, every entry point raises.
"""
import ctypes as C
import os

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblbk8s.so")
_PRODUCT_LIB = LIB_PATH
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
# csrc/Makefile's SRCS, in order: the library embeds the SHA-256 of their concatenation
SOURCES = ("lbk8s.hip", "lbk8s_common.h", "lbk8s_slice.h", "lbk8s_tpe.h", "lbk8s_rollout.h", "lbk8s_lean.h",
           "lbk8s_deepsets.h", "lbk8s_ds_train.h", "lbk8s_steps.h", "lbk8s_dqn.h", "lbk8s_ppo.h", "lbk8s_eval.h",
           "../../include/lbk8s.h",
           "lbk8s_lean_launch.h", "lbk8s_lean_inst.hip", "lbk8s_build.cpp")
ABI_VERSION = 17

LB_REWARD = {"naive": 0, "latency": 1, "fairness": 2, "multi": 3}
LB_RNG_PHILOX, LB_RNG_TRACE = 0, 1
LB_POLICY = {"topo": 0, "zone_cpu": 1, "endpoint_cpu": 2, "random": 3}
# lb_ds_forward_kernel's `which` (include/lbk8s.h LB_DS_FWD*)
LB_DS_FWD, LB_DS_FWD_TRAIN, LB_DS_FWD_ARGMAX, LB_DS_FWD_PAIR, LB_DS_FWD_SAMPLE = 0, 1, 2, 3, 5
# lb_rollout_kernel's answers (include/lbk8s.h LB_ROLLOUT_*)
LB_ROLLOUT = {0: "k_rollout_lean", 1: "k_rollout_img", 2: "k_rollout_tpe", 3: "policy+step launches",
              4: "k_rollout_slice", 5: "k_rollout_lean_split"}
LB_FIELD = {"endpoint_latency": 0, "endpoint_cpu_usage_percentage": 1,
            "endpoint_topology_latency": 2, "endpoint_zone_cpu_capacity": 3, "endpoint_zone": 4,
            "endpoint_node": 5, "avg_load_served": 6, "current_time": 7, "current_step": 8,
            "request_zone": 9, "request_threshold": 10}
PER_ENV_FIELDS = {"current_time", "current_step", "request_zone", "request_threshold"}
LB_ST_K = 16
LB_EPLOG_W = 24
LB_EPLOG_RET32, LB_EPLOG_REWARD, LB_EPLOG_ACTION, LB_EPLOG_ENV, LB_EPLOG_TAG = 16, 17, 18, 19, 20
LB_STATUS_BAD_ACTION, LB_STATUS_NOT_RESET = 1, 2
LB_PPO_STEPS_MAX = 4096  # lb_ppo_steps: vector steps per launch
LB_EVAL_STEPS_MAX = 4096  # lb_eval_steps: vector steps per launch
LB_GEOMETRY = {"auto": 0, "tpe": 1, "slice": 2}


class LBConfigC(C.Structure):
    _fields_ = [("num_endpoints", C.c_int32), ("num_zones", C.c_int32), ("num_nodes", C.c_int32),
                ("episode_length", C.c_int32), ("reward_fn", C.c_int32),
                ("rejection_allowed", C.c_int32), ("auto_reset", C.c_int32), ("rng_mode", C.c_int32),
                ("arrival_rate", C.c_double), ("call_duration", C.c_double),
                ("latency_weight", C.c_double), ("cpu_weight", C.c_double),
                ("gini_weight", C.c_double), ("seed", C.c_uint64), ("env_id_offset", C.c_int64),
                ("geometry", C.c_int32), ("reserved0", C.c_int32)]


TRACE_FIELDS = ["t0", "step_x1", "step_x2", "step_r", "step_n", "reset_lat0", "reset_topo",
                "reset_ntype", "reset_nzone", "reset_ncpu", "reset_enode", "reset_x1", "reset_x2",
                "reset_r", "reset_n"]


class LBTraceC(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in TRACE_FIELDS]


class LBDSWeightsC(C.Structure):
    """struct lb_ds_weights: device pointers to the torch parameters, as they are."""
    _fields_ = [("actor_lambda", C.c_void_p * 3), ("actor_gamma", C.c_void_p * 3),
                ("critic_lambda", C.c_void_p * 3), ("critic_gamma", C.c_void_p * 3),
                ("rho_w1", C.c_void_p), ("rho_b1", C.c_void_p), ("rho_w2", C.c_void_p),
                ("rho_b2", C.c_void_p)]


LB_DS_FRAG_FLOATS = 76872
LB_DS_MAX_ELEMENTS = 80       # forward held in registers (above: streamed in chunks)
LB_DS_MAX_ELEMENTS_TRAIN = 257  # training forward / backward, PPO loss head
LB_DS_MAX_ELEMENTS_FWD = 257  # inference forward / greedy argmax
LB_DS_BWD_FLOATS = 24704
LB_DS_SETVEC_FLOATS = 904
LB_DS_WGRAD_FLOATS = 4608
LB_DS_WORKSPACE_FLOATS = 1024 * 2 * LB_DS_WGRAD_FLOATS
LB_DS_OVER_SETS_SPAN = 256  # lb_ds_over_sets: sets per partial sum (workspace rows)
LB_DS_SETGRAD_ACTOR, LB_DS_SETGRAD_CRITIC = 4736, 12800
LB_DSV = {"MAX0": 0, "GA3": 8, "MAX2A": 72, "GS2A": 136, "MAX1A": 200, "GS1A": 264, "CS2": 328,
          "MAX2C": 392, "GS2C": 456, "MAX1C": 520, "GS1C": 584, "ID1A": 648, "ID2A": 680, "ID1C": 712,
          "ID2C": 744, "P1A": 776, "P1C": 840}


class LBDQNExploreC(C.Structure):
    """lb_dqn_explore (include/lbk8s.h)."""
    _fields_ = [("start_e", C.c_double), ("slope", C.c_double), ("end_e", C.c_double), ("seed", C.c_uint64),
                ("vstep_in", C.c_void_p), ("vstep_out", C.c_void_p), ("explore_out", C.c_void_p)]


class LBSetJobC(C.Structure):
    """lb_set_job (include/lbk8s.h): out[m][n] = scale * sum_s A(s, m) B(s, n)."""
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int64), ("b", C.c_void_p), ("ldb", C.c_int64), ("M", C.c_int32),
                ("N", C.c_int32), ("scale", C.c_float), ("out", C.c_void_p)]


_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


class StaleNativeLibrary(RuntimeError):
    pass


class NonDefaultBuild(StaleNativeLibrary):
    """A product library compiled with other flags than csrc/Makefile's defaults (a -D knob of
    a diagnostic build, another optimisation level): refused like a stale one."""


class _Tolerant:
    """A diagnostic library of another ABI: symbols it lacks become no-op stand-ins, so
    setting their argtypes does not fail (calling one raises)."""

    class _Missing:
        def __init__(self, name):
            self.name = name

        def __call__(self, *a):
            raise AttributeError(f"diagnostic library lacks {self.name}")

    def __init__(self, L):
        self.__dict__["_L"] = L

    def __getattr__(self, name):
        try:
            return getattr(self._L, name)
        except AttributeError:
            m = _Tolerant._Missing(name)
            self.__dict__[name] = m
            return m

    def __setattr__(self, name, value):
        setattr(self._L, name, value)


def source_hash():
    """First 16 hex digits of the SHA-256 of the library's sources (csrc/Makefile's SRC_HASH),
    or None where the sources are absent."""
    import hashlib
    h = hashlib.sha256()
    for f in SOURCES:
        path = os.path.normpath(os.path.join(CSRC, f))
        if not os.path.exists(path):
            return None
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _makefile_var(text, name):
    """The default (`NAME ?= ...`, continuation lines joined) of a variable of csrc/Makefile."""
    import re
    m = re.search(r"^" + name + r" \?= (.*?)(?<!\\)$", text, re.S | re.M)
    return " ".join(m.group(1).replace("\\\n", " ").split()) if m else ""


def expected_build_flags():
    """The flags csrc/Makefile compiles a product library with (HIPFLAGS with $(ARCH)
    expanded, no DEFS), whitespace-normalised; None where the Makefile is absent."""
    path = os.path.join(CSRC, "Makefile")
    if not os.path.exists(path):
        return None
    with open(path) as fh:
        text = fh.read()
    flags = _makefile_var(text, "HIPFLAGS").replace("$(ARCH)", _makefile_var(text, "ARCH"))
    return " ".join(flags.split())


def build_hash(L):
    """First 16 hex digits of SHA-256(source hash, flags, compiler) of a loaded library: one
    word for the whole build (smoke prints it)."""
    import hashlib
    parts = [L.lb_source_hash(), L.lb_build_flags(), L.lb_build_compiler()]
    return hashlib.sha256(b"\n".join(parts)).hexdigest()[:16]


def lib():
    """Load liblbk8s.so (once). Raises NativeLibraryMissing if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (share torch's HIP runtime, see module docstring)
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: build it with `make -C gym-loadbalancing_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    product = os.path.abspath(LIB_PATH) == _PRODUCT_LIB
    if not product:  # a diagnostic build (tools/ A/B runs): an older ABI may lack symbols
        L = _Tolerant(L)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    cfgp = C.POINTER(LBConfigC)
    trp = C.POINTER(LBTraceC)
    L.lb_abi_version.restype = C.c_int
    L.lb_last_error.restype = C.c_char_p
    L.lb_validate_config.argtypes = [cfgp]
    L.lb_state_bytes.argtypes = [cfgp, i64, C.POINTER(C.c_uint64)]
    L.lb_init.argtypes = [vp, cfgp, i64, trp, vp]
    L.lb_reset.argtypes = [vp, cfgp, i64, vp, vp, trp, vp]
    L.lb_step.argtypes = [vp, cfgp, i64, vp, vp, vp, vp, vp, vp, trp, vp]
    L.lb_policy.argtypes = [vp, cfgp, i64, i32, vp, vp]
    L.lb_rollout.argtypes = [vp, cfgp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.lb_rollout_kernel.argtypes = [cfgp, i64, i32, i32, C.POINTER(C.c_int32)]
    L.lb_get_field.argtypes = [vp, cfgp, i64, i32, vp, vp]
    L.lb_get_stats.argtypes = [vp, cfgp, i64, vp, vp]
    L.lb_status.argtypes = [vp, cfgp, i64, vp, vp]
    L.lb_ds_pack.argtypes = [C.POINTER(LBDSWeightsC), vp, vp]
    L.lb_ds_forward.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.lb_ds_q_argmax.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    L.lb_ds_sample.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    f32 = C.c_float
    L.lb_ppo_head.argtypes = [vp] * 8 + [i64, i32, f32, f32, f32, i32, vp, vp, vp, vp]
    L.lb_replay_add.argtypes = [i64, i32, i64] + [vp] * 15 + [vp]
    L.lb_ds_train_forward.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, vp]
    L.lb_ds_pack_backward.argtypes = [C.POINTER(LBDSWeightsC), vp, vp]
    L.lb_ds_forward_pair.argtypes = [vp] * 8 + [i64, i32, vp]
    L.lb_ds_forward_kernel.argtypes = [i32, i64, i32] + [C.POINTER(C.c_int32)] * 3
    L.lb_ds_pack_pair.argtypes = [C.POINTER(LBDSWeightsC), vp, vp, vp]
    L.lb_ds_train_backward.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lb_episode_log.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp]
    L.lb_ppo_record.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp]
    L.lb_gae.argtypes = [vp] * 5 + [i64, i64, C.c_double, C.c_double, vp, vp, vp]
    L.lb_ppo_steps_supported.argtypes = [cfgp, i64, i32]
    L.lb_ppo_steps.argtypes = [vp, vp, vp, cfgp, i64, i32, i32, i32] + [vp] * 16 + [i64, vp, i64, vp, vp]
    L.lb_eval_steps_supported.argtypes = [cfgp, i64, i32]
    L.lb_eval_steps.argtypes = [vp, vp, vp, cfgp, i64, i32, vp, i32] + [vp] * 11 + [i64, vp, i64, vp, vp]
    L.lb_reward64.argtypes = [vp, cfgp, i64, C.POINTER(C.c_void_p)]
    L.lb_dqn_act.argtypes = [vp, vp, i64, i32, vp, vp, cfgp, C.POINTER(LBDQNExploreC), vp, vp]
    L.lb_dqn_step.argtypes = [vp, vp, i64, i32, vp, vp, cfgp, C.POINTER(LBDQNExploreC), vp, vp, vp, vp, vp, vp,
                              i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lb_dqn_steps.argtypes = L.lb_dqn_step.argtypes[:-1] + [i32, vp, vp]
    L.lb_dqn_steps_supported.argtypes = [cfgp, i64, i32]
    L.lb_dqn_head.argtypes = [vp, vp, vp, vp, vp, i64, i32, C.c_float, vp, vp, vp, vp, vp, vp]
    L.lb_replay_sample.argtypes = [i64, i32, i64, i32, C.c_uint64] + [vp] * 12 + [vp]
    L.lb_ds_set_grads.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.lb_ds_train_backward_sets.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lb_ds_over_sets.argtypes = [C.POINTER(LBSetJobC), i32, i64, vp, i64, vp]
    for f in ("lb_validate_config", "lb_state_bytes", "lb_init", "lb_reset", "lb_step", "lb_policy", "lb_rollout",
              "lb_rollout_kernel", "lb_reward64",
              "lb_get_field", "lb_get_stats", "lb_status", "lb_ds_pack", "lb_ds_forward",
              "lb_ds_train_forward", "lb_ds_pack_backward", "lb_ds_train_backward", "lb_ds_q_argmax",
              "lb_replay_add", "lb_ppo_head", "lb_episode_log", "lb_dqn_act", "lb_dqn_head",
              "lb_replay_sample", "lb_ds_set_grads", "lb_dqn_step", "lb_dqn_steps",
              "lb_dqn_steps_supported", "lb_ds_pack_pair", "lb_ds_forward_pair", "lb_ds_over_sets",
              "lb_ds_train_backward_sets", "lb_ds_forward_kernel", "lb_ds_sample", "lb_ppo_record", "lb_gae",
              "lb_ppo_steps_supported", "lb_ppo_steps", "lb_eval_steps_supported", "lb_eval_steps"):
        getattr(L, f).restype = C.c_int
    v = L.lb_abi_version()
    if v != ABI_VERSION and product:
        raise RuntimeError(f"liblbk8s.so ABI {v} != expected {ABI_VERSION}; rebuild it")
    if product:  # (another LIB_PATH: a diagnostic build of other sources, tools/ only)
        for f in ("lb_source_hash", "lb_build_flags", "lb_build_compiler"):
            getattr(L, f).restype = C.c_char_p
        built, now = L.lb_source_hash().decode(), source_hash()
        if now is not None and built != now:
            raise StaleNativeLibrary(f"{LIB_PATH} was built from sources {built}, the tree's are {now}: "
                                     "rebuild it (make -C gym-loadbalancing_amd/csrc, or __graft_entry__.build())")
        flags, want = " ".join(L.lb_build_flags().decode().split()), expected_build_flags()
        if want is not None and flags != want:
            raise NonDefaultBuild(f"{LIB_PATH} was built with flags '{flags}', csrc/Makefile's defaults are "
                                  f"'{want}': a diagnostic build is not the product (rebuild with make -B)")
    _lib = L
    return L


def check(rc):
    """Raise on a non-zero return code, mirroring the reference's exception types."""
    if rc == 0:
        return
    msg = lib().lb_last_error().decode()
    if msg.startswith("IndexError"):
        raise IndexError(msg)
    raise RuntimeError(f"liblbk8s: {msg} (rc={rc})")


EXPORTED_SYMBOLS = ("lb_abi_version", "lb_last_error", "lb_validate_config", "lb_state_bytes",
                    "lb_init", "lb_reset", "lb_step", "lb_policy", "lb_rollout", "lb_get_field", "lb_get_stats",
                    "lb_status", "lb_ds_pack", "lb_ds_forward", "lb_ds_train_forward",
                    "lb_ds_pack_backward", "lb_ds_train_backward", "lb_ds_q_argmax", "lb_replay_add", "lb_ppo_head",
                    "lb_episode_log", "lb_dqn_act", "lb_dqn_head", "lb_replay_sample", "lb_ds_set_grads",
                    "lb_rollout_kernel", "lb_source_hash", "lb_build_flags", "lb_build_compiler", "lb_reward64",
                    "lb_dqn_step",
                    "lb_dqn_steps", "lb_dqn_steps_supported", "lb_ds_pack_pair", "lb_ds_forward_pair",
                    "lb_ds_over_sets", "lb_ds_train_backward_sets", "lb_ds_forward_kernel", "lb_ds_sample",
                    "lb_ppo_record", "lb_gae", "lb_ppo_steps_supported", "lb_ppo_steps",
                    "lb_eval_steps_supported", "lb_eval_steps")
