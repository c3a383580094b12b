"""The order of things in a sampler call, host-side only (no GPU, no libeodiff.so): the walk over a resampling schedule, the Philox
stream numbering that goes with it, and the picking of injected draws.  EODiffusion.sampling / sampling_scene and DDIMSampler.
ddim_sampling / sample_scene hand `walk` their step and jump bodies as callables; the walk never asks which sampler called it.

Philox keys of a chain (seed, sample index, step, stream id): x_T is (step T, stream X_T_STREAM); evaluation number v = 0, 1, ... of
level i draws its mix / step noise with (step i, stream step_stream(v)); the jump that lands on level b, which b has been evaluated
n >= 1 times before, with (step b, stream jump_stream(n)).  Odd streams are steps, even ones moves: no two draws share a key."""
try:
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(it, **kw):
        return it

X_T_STREAM = 0


def step_stream(visit):
    return 1 + 2 * visit


def jump_stream(visits_of_b):
    return 2 * visits_of_b


def pick(draws, k):
    """entry k of injected draws: a tensor / list, or a callable k -> tensor"""
    return draws(k) if callable(draws) else draws[k]


def walk(x, visits, jump_after, step, jump, desc=None):
    """Walk util.resample_plan's (visits, jump_after) from the state x: x = step(x, k, level, visit) for evaluation number k = 0, 1, ...
    at `level`, visit = how many evaluations of that level came before; after evaluation number k + 1 in jump_after = {k + 1: (j, a, b)}
    x = jump(x, j, a, b, visits_of_b), the evaluations of level b so far.  desc: the title of a tqdm bar, None for no bar."""
    seen = {}  # level -> evaluations so far
    it = tqdm(visits, desc=desc, total=len(visits)) if desc else visits
    for k, level in enumerate(it):
        visit = seen.get(level, 0)
        seen[level] = visit + 1
        x = step(x, k, level, visit)
        if k + 1 in jump_after:
            j, a, b = jump_after[k + 1]
            x = jump(x, j, a, b, seen[b])
    return x
