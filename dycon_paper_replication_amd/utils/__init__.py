from . import dycon_losses, losses, monitor, ramps  # noqa: F401
from . import sliding_window, test_3d_patch  # noqa: F401

# utils/test_3d_patch.py holds the evaluator as it was written for 2-class models and is kept as it is; 2-class nets still run
# through it.  The reference's test_single_case takes any class count (code/utils/test_3d_patch.py:293-351), so the package binds
# the class-count form (utils/sliding_window.py, which hands 2-class nets to the original) under that name: test_all_case, the
# var_all_case_* / test_all_case_* wrappers and every caller of utils.test_3d_patch.test_single_case resolve it at call time.
test_3d_patch.test_single_case = sliding_window.test_single_case

# the all-class evaluator and the per-class metrics come beside it under names of their own and rebind nothing
from . import eval_classes  # noqa: E402,F401
from . import surface  # noqa: E402,F401
from . import surface_eval  # noqa: E402,F401
from . import components  # noqa: E402,F401
from . import device_eval  # noqa: E402,F401
from . import lesions  # noqa: E402,F401
from . import isles_eval  # noqa: E402,F401
from . import util  # noqa: E402,F401

# the reference's two-model (`_plus`) evaluators, its LA validation loops and two small helpers (code/utils/test_3d_patch.py:14-17,
# :28-49, :354-476, :488-494) live in utils/ensemble_eval.py; test_3d_patch.py had none of them, so binding them there rebinds nothing
from . import ensemble_eval  # noqa: E402,F401

for _name in ensemble_eval.REFERENCE_NAMES:
    setattr(test_3d_patch, _name, getattr(ensemble_eval, _name))
del _name
