from linetr_amd.evaluations import Evaluate_PR  # noqa: F401
