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
SOURCES = ("lbk8s_env_steps.hip", "lbk8s_env.hip", "lbk8s_ds.hip", "lbk8s_ds_train.hip", "lbk8s_steps.hip",
           "lbk8s_learn.hip", "lbk8s_host.h", "lbk8s_common.h", "lbk8s_slice.h", "lbk8s_tpe.h", "lbk8s_rollout.h", "lbk8s_lean.h",
           "lbk8s_deepsets.h", "lbk8s_ds_chunked.h", "lbk8s_ds_train.h", "lbk8s_steps.h", "lbk8s_dqn.h", "lbk8s_ppo.h", "lbk8s_eval.h",
           "../../include/lbk8s.h", "../../include/lbk8s_abi_steps64.h", "../../include/lbk8s_abi_dqn64.h",
           "../../include/lbk8s_abi_steps256.h", "../../include/lbk8s_abi_dqn256.h", "../../include/lbk8s_abi_ppo256.h", "../../include/lbk8s_abi_ppo_tl.h",
           "lbk8s_lean_launch.h", "lbk8s_lean_inst.hip", "lbk8s_policies.hip", "lbk8s_steps64.h", "lbk8s_dqn64.h",
           "lbk8s_steps64.hip", "lbk8s_steps256.h", "lbk8s_dqn256.h", "lbk8s_ppo256.h", "lbk8s_steps256.hip", "lbk8s_steps_host.h",
           "lbk8s_build.cpp")
ABI_VERSION = 17

LB_REWARD = {"naive": 0, "latency": 1, "fairness": 2, "multi": 3}
LB_RNG_PHILOX, LB_RNG_TRACE = 0, 1
LB_POLICY = {"topo": 0, "zone_cpu": 1, "endpoint_cpu": 2, "random": 3,
             "round_robin": 4, "least_loaded": 5, "least_latency": 6, "reward_greedy": 7}
# kinds without lean / image rollout kernels (lb_rollout runs k_rollout_tpe in their place)
POLICIES_WITHOUT_LEAN_KERNELS = ("round_robin", "least_loaded", "least_latency", "reward_greedy")
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


def _prototypes():
    """include/lbk8s.h's prototypes, name -> (restype, argtypes): the one place a signature is
    written (tests/test_native_abi.py compares it with the header, argument by argument)."""
    vp, i64, i32, u64, f32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_float, C.c_double
    cfgp, trp, wp, exp = C.POINTER(LBConfigC), C.POINTER(LBTraceC), C.POINTER(LBDSWeightsC), C.POINTER(LBDQNExploreC)
    i32p = C.POINTER(i32)
    # lb_dqn_step up to ep_cnt (lb_dqn_steps continues with steps and sync)
    dqn_step = [vp, vp, i64, i32, vp, vp, cfgp, exp] + [vp] * 6 + [i64] + [vp] * 9
    # lb_ppo_record's / lb_ppo_steps' / lb_eval_steps' tail: tag, log, cap, count, stream
    log_tail = [i64, vp, i64, vp, vp]
    ints = {
        "lb_abi_version": [],
        "lb_validate_config": [cfgp],
        "lb_state_bytes": [cfgp, i64, C.POINTER(u64)],
        "lb_init": [vp, cfgp, i64, trp, vp],
        "lb_reset": [vp, cfgp, i64, vp, vp, trp, vp],
        "lb_step": [vp, cfgp, i64] + [vp] * 6 + [trp, vp],
        "lb_rollout": [vp, cfgp, i64, i32, i32] + [vp] * 7,
        "lb_rollout_kernel": [cfgp, i64, i32, i32, i32p],
        "lb_policy": [vp, cfgp, i64, i32, vp, vp],
        "lb_get_field": [vp, cfgp, i64, i32, vp, vp],
        "lb_get_stats": [vp, cfgp, i64, vp, vp],
        "lb_status": [vp, cfgp, i64, vp, vp],
        "lb_ds_pack": [wp, vp, vp],
        "lb_ds_forward": [vp, vp, i64, i32, vp, vp, vp],
        "lb_ds_q_argmax": [vp, vp, i64, i32] + [vp] * 4,
        "lb_ds_sample": [vp, vp, i64, i32] + [vp] * 8,
        "lb_replay_add": [i64, i32, i64] + [vp] * 16,
        "lb_dqn_act": [vp, vp, i64, i32, vp, vp, cfgp, exp, vp, vp],
        "lb_dqn_step": dqn_step + [vp],
        "lb_dqn_steps_supported": [cfgp, i64, i32],
        "lb_dqn_steps": dqn_step + [i32, vp, vp],
        "lb_dqn_head": [vp] * 5 + [i64, i32, f32] + [vp] * 6,
        "lb_replay_sample": [i64, i32, i64, i32, u64] + [vp] * 13,
        "lb_reward64": [vp, cfgp, i64, C.POINTER(vp)],
        "lb_episode_log": [i64] + [vp] * 7 + log_tail,
        "lb_ppo_record": [i64] + [vp] * 10 + log_tail,
        "lb_gae": [vp] * 5 + [i64, i64, f64, f64, vp, vp, vp],
        "lb_ppo_steps_supported": [cfgp, i64, i32],
        "lb_ppo_steps": [vp, vp, vp, cfgp, i64, i32, i32, i32] + [vp] * 16 + log_tail,
        "lb_eval_steps_supported": [cfgp, i64, i32],
        "lb_eval_steps": [vp, vp, vp, cfgp, i64, i32, vp, i32] + [vp] * 11 + log_tail,
        "lb_ds_train_forward": [vp, vp, i64, i32] + [vp] * 6,
        "lb_ds_forward_pair": [vp] * 8 + [i64, i32, vp],
        "lb_ds_forward_kernel": [i32, i64, i32, i32p, i32p, i32p],
        "lb_ppo_head": [vp] * 8 + [i64, i32, f32, f32, f32, i32, vp, vp, vp, vp],
        "lb_ds_pack_backward": [wp, vp, vp],
        "lb_ds_pack_pair": [wp, vp, vp, vp],
        "lb_ds_train_backward": [vp, vp, i64, i32] + [vp] * 8,
        "lb_ds_set_grads": [vp, vp, vp, i64, i32, vp, vp],
        "lb_ds_train_backward_sets": [vp, vp, i64, i32] + [vp] * 9,
        "lb_ds_over_sets": [C.POINTER(LBSetJobC), i32, i64, vp, i64, vp],
    }
    protos = {name: (C.c_int, args) for name, args in ints.items()}
    for name in ("lb_last_error", "lb_source_hash", "lb_build_flags", "lb_build_compiler"):
        protos[name] = (C.c_char_p, [])
    return protos


PROTOTYPES = _prototypes()
EXPORTED_SYMBOLS = tuple(PROTOTYPES)
# include/lbk8s_abi_steps64.h's prototypes (lbk8s.h includes it): the twins' signatures
# (tests/test_steps64_host.py compares this table with that header, as test_native_abi.py the other)
STEPS64_PROTOTYPES = {name.replace("_steps", "_steps64"): PROTOTYPES[name]
                      for name in ("lb_ppo_steps_supported", "lb_ppo_steps", "lb_eval_steps_supported", "lb_eval_steps")}
STEPS64_SYMBOLS = tuple(STEPS64_PROTOTYPES)
# include/lbk8s_abi_dqn64.h's prototypes (lbk8s.h includes it too): lb_dqn_steps' twin
# (tests/test_dqn_steps64_host.py compares this table with that header)
DQN64_PROTOTYPES = {name.replace("_steps", "_steps64"): PROTOTYPES[name]
                    for name in ("lb_dqn_steps_supported", "lb_dqn_steps")}
DQN64_SYMBOLS = tuple(DQN64_PROTOTYPES)
# include/lbk8s_abi_steps256.h's prototypes (lbk8s.h includes it too): lb_eval_steps' twin for envs
# of up to 256 endpoints (tests/test_steps256_host.py compares this table with that header)
STEPS256_PROTOTYPES = {name.replace("_steps", "_steps256"): PROTOTYPES[name]
                       for name in ("lb_eval_steps_supported", "lb_eval_steps")}
STEPS256_SYMBOLS = tuple(STEPS256_PROTOTYPES)
# include/lbk8s_abi_dqn256.h's prototypes (lbk8s.h includes it too): lb_dqn_steps' twin for envs of
# up to 256 endpoints (tests/test_dqn_steps256_host.py compares this table with that header)
DQN256_PROTOTYPES = {name.replace("_steps", "_steps256"): PROTOTYPES[name]
                     for name in ("lb_dqn_steps_supported", "lb_dqn_steps")}
DQN256_SYMBOLS = tuple(DQN256_PROTOTYPES)
# include/lbk8s_abi_ppo256.h's prototypes (lbk8s.h includes it last): lb_ppo_steps' twin for envs of
# up to 256 endpoints (tests/test_ppo_steps256_host.py compares this table with that header)
PPO256_PROTOTYPES = {name.replace("_steps", "_steps256"): PROTOTYPES[name]
                     for name in ("lb_ppo_steps_supported", "lb_ppo_steps")}
PPO256_SYMBOLS = tuple(PPO256_PROTOTYPES)


def _ppo_tl_prototypes():
    """include/lbk8s_abi_ppo_tl.h's prototypes (lbk8s_abi_ppo256.h includes it): PPO's value targets
    that bootstrap from the terminal state at a time limit (tests/test_ppo_tl_host.py compares this
    table with that header).  lb_gae_tl: lb_gae with term_values after next_done; lb_ppo_steps_tl:
    lb_ppo_steps with terminal_obs and term_values before the stream."""
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    gae, steps = PROTOTYPES["lb_gae"][1], PROTOTYPES["lb_ppo_steps"][1]
    return {"lb_gae_tl": (C.c_int, gae[:5] + [vp] + gae[5:]),
            "lb_ds_value_where": (C.c_int, [vp, vp, vp, i64, i32, vp, vp]),
            "lb_ppo_steps_tl_supported": PROTOTYPES["lb_ppo_steps_supported"],
            "lb_ppo_steps_tl": (C.c_int, steps[:-1] + [vp, vp] + steps[-1:])}


PPO_TL_PROTOTYPES = _ppo_tl_prototypes()
PPO_TL_SYMBOLS = tuple(PPO_TL_PROTOTYPES)

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
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)  # (a diagnostic library's stand-in where it lacks the symbol)
        f.restype, f.argtypes = restype, argtypes
    for name, (restype, argtypes) in {**STEPS64_PROTOTYPES, **DQN64_PROTOTYPES, **STEPS256_PROTOTYPES,
                                       **DQN256_PROTOTYPES, **PPO256_PROTOTYPES, **PPO_TL_PROTOTYPES}.items():
        # (a product library is built from the tree's sources, checked below, and has them; in any
        # other, calling one raises: there is no stand-in and no fallback)
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    v = L.lb_abi_version()
    if v != ABI_VERSION and product:
        raise RuntimeError(f"liblbk8s.so ABI {v} != expected {ABI_VERSION}; rebuild it")
    if product:  # (another LIB_PATH: a diagnostic build of other sources, tools/ only)
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
