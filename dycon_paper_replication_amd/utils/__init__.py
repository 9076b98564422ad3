from . import dycon_losses, losses, monitor, ramps  # noqa: F401
