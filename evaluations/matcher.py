from linetr_amd.evaluations import nn_matcher_batches  # noqa: F401
