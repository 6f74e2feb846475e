"""One tournament round on the device (tournament.rs), host side only.

    round_robin_pods        tournament.rs:918-920
    swiss_points            tournament.rs:715-750 calculate_swiss_points
    run_round               the pods of a round through bppo.eval.evaluate_pods; per pod the
                            MatchupGames content of run_pod (tournament.rs:1788-1870)

    find_anchor_index       tournament.rs:1017-1033
    rate_round              compute_ratings(contestants, all_games), tournament.rs:1035-1049, on a
                            device rating table (bppo.ratings)

Every pod of a round has its own RNG (evaluate_pods), where the reference hands one StdRng
from pod to pod.  Pairing for Swiss rounds (swiss_pods, form_dutch_pods*), the graphs and
checkpoint discovery on disk are not part of this module."""
import itertools

from .eval import evaluate_pods
from .ratings import RatingTable


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


def find_anchor_index(names):
    """the anchor of a tournament's ratings: the contestant called "Random" if there is one, else
    the "step_*" contestant with the smallest name (the first of equal ones), else None"""
    for i, n in enumerate(names):
        if n == "Random":
            return i
    best = None
    for i, n in enumerate(names):
        if n.startswith("step_") and (best is None or n < names[best]):
            best = i
    return best


def rate_round(results, n_contestants, anchor, table=None, random_index=None, config=None, device=0,
               backend="device"):
    """Append the games of run_round's output to a rating table and fit it over n_contestants
    players: a pod's contestant indices are the player ids as they are; a None contestant (the
    random player) is player random_index, as the caller numbers it.  table: a RatingTable that
    already holds the earlier rounds' games (the reference refits over all games after every
    round, tournament.rs:2250); None = a table of this call's own.  -> RatingResult"""
    own = table is None
    if own:
        table = RatingTable(device=device)
    try:
        players, placements = [], []
        for pod in results:
            ids = []
            for c in pod["contestants"]:
                if c is None:
                    if random_index is None:
                        raise ValueError("rate_round: a pod seats the random player (None); give random_index")
                    c = random_index
                ids.append(int(c))
            for game in pod["games"]:
                players.append(ids)
                placements.append([int(p) for p in game])
        table.add_games(players, placements)
        return table.fit(n_contestants, anchor, config, backend)
    finally:
        if own:
            table.close()
