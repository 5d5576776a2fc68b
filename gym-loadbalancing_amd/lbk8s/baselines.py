"""Greedy heuristic policies of envs/baselines.py:6-35.

Host form (same signatures, any env exposing the attributes): feasible endpoints are the
True entries of action_mask[:-1]; the last mask entry is dropped whether or not it is
the reject action (so without rejection the last endpoint is never chosen, as in the
reference); ties go to the lowest index (numpy argmin/argmax); with no feasible
endpoint the last action index is returned.

Batched device form: LBVecEnv.policy("topo" | "zone_cpu" | "endpoint_cpu") — the same
rule evaluated by k_policy for every env at once (masks are always all True, :808-821).

K8S_POLICIES: the baselines a Kubernetes load balancer ships, which are not the reference's
(LB_POLICY_ROUND_ROBIN, LEAST_LOADED, LEAST_LATENCY; device form LBVecEnv.policy("round_robin" |
"least_loaded" | "least_latency")).  They consider all E endpoints, never reject, and so do not
inherit the mask[:-1] quirk above: the last endpoint is eligible without rejection.  Ties go to
the lowest index.  The fourth device kind, "reward_greedy", has no host form: it needs the step.
"""
import numpy as np


def _pick(values, action_mask, largest):
    feasible = np.flatnonzero(np.asarray(action_mask)[:-1])
    if feasible.size == 0:
        return len(action_mask) - 1
    v = np.asarray(values)[feasible]
    return int(feasible[np.argmax(v) if largest else np.argmin(v)])


def topology_greedy_policy(env, action_mask):
    """Feasible endpoint with the lowest topology latency to the request (:6-13)."""
    return _pick(env.endpoint_topology_latency, action_mask, largest=False)


def zone_cpu_greedy_policy(env, action_mask):
    """Feasible endpoint whose zone has the largest cpu capacity (:16-24)."""
    return _pick(env.endpoint_zone_cpu_capacity, action_mask, largest=True)


def endpoint_cpu_greedy_policy(env, action_mask):
    """Feasible endpoint with the lowest cpu usage (:27-35)."""
    return _pick(env.endpoint_cpu_usage_percentage, action_mask, largest=False)


POLICIES = {"topo": topology_greedy_policy, "zone_cpu": zone_cpu_greedy_policy,
            "endpoint_cpu": endpoint_cpu_greedy_policy}


def round_robin_policy(env, action_mask):
    """IPVS rr: endpoint current_step mod E (current_step counts the episode's steps so far)."""
    return int(env.current_step) % len(env.avg_load_served)


def least_loaded_policy(env, action_mask):
    """IPVS lc: the endpoint that served the fewest requests this episode (avg_load_served)."""
    return int(np.argmin(np.asarray(env.avg_load_served)))


def least_latency_policy(env, action_mask):
    """The endpoint with the lowest endpoint latency + topology latency to the request's zone,
    one float64 add per endpoint: the sum the latency and multi rewards pay for."""
    lat = np.asarray(env.endpoint_latency, dtype=np.float64)
    topo = np.asarray(env.endpoint_topology_latency).astype(np.float64)
    return int(np.argmin(lat + topo))


K8S_POLICIES = {"round_robin": round_robin_policy, "least_loaded": least_loaded_policy,
                "least_latency": least_latency_policy}
