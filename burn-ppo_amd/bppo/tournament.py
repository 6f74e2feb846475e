"""One tournament round on the device (tournament.rs), host side only.

    round_robin_pods        tournament.rs:918-920
    swiss_points            tournament.rs:715-750 calculate_swiss_points
    run_round               the pods of a round through bppo.eval.evaluate_pods; per pod the
                            MatchupGames content of run_pod (tournament.rs:1788-1870)

Every pod of a round has its own RNG (evaluate_pods), where the reference hands one StdRng
from pod to pod.  Pairing for Swiss rounds, ratings and graphs are not part of this module."""
import itertools

from .eval import evaluate_pods


def round_robin_pods(n, pod_size):
    """every combination of pod_size contestants out of n, in lexicographic order"""
    return [list(p) for p in itertools.combinations(range(n), pod_size)]


def swiss_points(placements):
    """points of one game by fractional ranking: N - the average of the positions a tie group
    occupies.  [1, 1, 3, 4] -> [2.5, 2.5, 1.0, 0.0]"""
    n = len(placements)
    counts = {}
    for p in placements:
        counts[p] = counts.get(p, 0) + 1
    avg, pos = {}, 1
    for p in sorted(counts):
        avg[p] = (pos + (pos + counts[p] - 1)) / 2.0
        pos += counts[p]
    return [float(n) - avg[p] for p in placements]


def run_round(config, models, normalizers, pods, num_games, envs_per_pod, temp_schedule=None, seeds=None, seed=0,
              device=0, max_steps=None):
    """pods[k]: the contestants of pod k, indices into models (None = the random player).
    -> per pod {"contestants": pods[k], "games": [placements of each game, per contestant],
    "stats": its EvalStats}"""
    stats = evaluate_pods(config, models, normalizers, pods, num_games, envs_per_pod, temp_schedule, seeds, seed,
                          device, max_steps)
    return [{"contestants": list(pod), "games": [list(o) for o in st.game_outcomes], "stats": st}
            for pod, st in zip(pods, stats)]
