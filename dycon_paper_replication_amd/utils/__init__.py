from . import dycon_losses, losses, monitor, ramps  # noqa: F401
from . import sliding_window, test_3d_patch  # noqa: F401

# test_3d_patch.py imports test_single_case from sliding_window.py, so this holds already.  It is stated here once more for a
# test_3d_patch.py of the earlier layout, which defined a 2-class function of that name in the file: with one of those on the path
# the reference's name must still be the class-count evaluator for test_all_case and the var_all_case_* / test_all_case_* wrappers
test_3d_patch.test_single_case = sliding_window.test_single_case

from . import case_loop  # noqa: E402,F401
from . import eval_classes  # noqa: E402,F401
from . import surface  # noqa: E402,F401
from . import surface_eval  # noqa: E402,F401
from . import components  # noqa: E402,F401
from . import morphology  # noqa: E402,F401
from . import device_eval  # noqa: E402,F401
from . import lesions  # noqa: E402,F401
from . import isles_eval  # noqa: E402,F401
from . import util  # noqa: E402,F401
from . import uncertainty  # noqa: E402,F401
from . import filters  # noqa: E402,F401

# the reference's two-model (`_plus`) evaluators, its LA validation loops and two small helpers (code/utils/test_3d_patch.py:14-17,
# :28-49, :354-476, :488-494) live in utils/ensemble_eval.py, which imports test_3d_patch.py; they get the reference's module here
from . import ensemble_eval  # noqa: E402,F401

for _name in ensemble_eval.REFERENCE_NAMES:
    setattr(test_3d_patch, _name, getattr(ensemble_eval, _name))
del _name
