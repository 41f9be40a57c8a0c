"""Import-path shim: the reference's train.py does ``from evaluations import criteria`` and ``from evaluations.metric import
Result``; these modules forward to the MI355X-native implementation in ``linetr_amd.evaluations`` -- see INTEGRATION.md."""
