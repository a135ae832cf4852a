"""tfa.optimizers.LAMB as the legacy Trainer of the reference selects it (trainer.py:31-38: `tfa.optimizers.LAMB(learning_rate=self.lr0)`).

`LAMB(...)` mirrors tensorflow_addons' constructor and holds hyperparameters only; `Trainer(model, optimizer=LAMB(...))` selects
the kernels of csrc/lamb.hip.  A "variable" is one ParamSpec of the engine: its trust ratio ||w|| / ||u|| is taken over the
parameter's own elements (zero-padded channels and the alignment tail of its slot add exactly zero).

PARITY UNPINNED: tensorflow_addons is not available to this project; the arithmetic restates `_resource_apply_dense` of
tensorflow_addons/optimizers/lamb.py and is held to an fp64 restatement (tests/lamb_ref.py)."""
import re


class LAMB:
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-6, weight_decay=0.0, exclude_from_weight_decay=None,
                 exclude_from_layer_adaptation=None):
        """exclude_from_weight_decay / exclude_from_layer_adaptation: lists of regular expressions, `re.search`ed against the
        parameter names; the second defaults to the first, as in tfa."""
        self.learning_rate = float(learning_rate)
        self.beta_1, self.beta_2, self.epsilon, self.weight_decay = float(beta_1), float(beta_2), float(epsilon), float(weight_decay)
        self.exclude_from_weight_decay = None if exclude_from_weight_decay is None else list(exclude_from_weight_decay)
        if exclude_from_layer_adaptation is None:
            exclude_from_layer_adaptation = self.exclude_from_weight_decay
        self.exclude_from_layer_adaptation = None if exclude_from_layer_adaptation is None else list(exclude_from_layer_adaptation)

    @staticmethod
    def _excluded(name, patterns):
        return bool(patterns) and any(re.search(p, name) is not None for p in patterns)

    def decayed(self, name):
        """tfa's _do_use_weight_decay."""
        return not self._excluded(name, self.exclude_from_weight_decay)

    def adapted(self, name):
        """tfa's _do_layer_adaptation."""
        return not self._excluded(name, self.exclude_from_layer_adaptation)

    def segments(self, specs):
        """(offset, real element count, slot length, decayed, adapted) per ParamSpec, in buffer order: the rows of ops.LambTable."""
        return [(s_.offset, s_.numel, s_.end - s_.offset, self.decayed(n), self.adapted(n)) for n, s_ in specs.items()]

    def get_config(self):
        return {"learning_rate": self.learning_rate, "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "weight_decay": self.weight_decay, "exclude_from_weight_decay": self.exclude_from_weight_decay,
                "exclude_from_layer_adaptation": self.exclude_from_layer_adaptation}
