from linetr_amd.evaluations import AverageMeter, Evaluate_PR, Result, nn_matcher_batches  # noqa: F401
