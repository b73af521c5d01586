"""The one way the tests set an SD_* environment variable: around a block, with what was there before put back after it -
the developer's own exported value, or "not set"."""
import contextlib
import os


@contextlib.contextmanager
def tunables(env=None, **more):
    """A session keeps the planner tunables of its creation, the session-less entries (sd_gemm_route, sd_gemm_bf16, the row
    limits) and the per-call switches read theirs at the call: set them around the creation / the call.  Values are
    str()-ed; None leaves the variable unset inside the block."""
    env = dict(env or {}, **more)
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
