"""Training on the device: the loss of one minibatch of an LSTM decoder's windows and its gradient with respect to the
weights, from the uint8 counts where they lie (libmuahuff_train.so, include/muahuff_train.h).  The call itself is
lstm.loss_and_grad; LSTMDecoder.fit(engine="device") and lstm.cross_validate(..., engine="device") train through it with
torch's optimizers.  There is no CPU path."""
from ._train import MAX_BATCH, scratch_bytes, scratch_layout  # noqa: F401
from .lstm import loss_and_grad  # noqa: F401
