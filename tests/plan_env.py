"""Environment knobs the planner reads at plan creation, set around a block (shared by the GPU tests)."""
import contextlib


class plan_mode:
    """VXG_PLAN_BATCH for the plans created inside (plan.hip reads it at every vxg_plan_create):
    "0" unbatched, "1" batched, "mixed", None = the default (plain create: the batched
    candidate; measure=True: both recorded, vxg_plan_select keeps one)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        import os
        self.old = os.environ.get("VXG_PLAN_BATCH")
        if self.mode is None:
            os.environ.pop("VXG_PLAN_BATCH", None)
        else:
            os.environ["VXG_PLAN_BATCH"] = self.mode

    def __exit__(self, *exc):
        import os
        if self.old is None:
            os.environ.pop("VXG_PLAN_BATCH", None)
        else:
            os.environ["VXG_PLAN_BATCH"] = self.old


@contextlib.contextmanager
def env_set(**kv):
    """Environment variables set for the block (the planner reads these at plan recording)."""
    import os
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
