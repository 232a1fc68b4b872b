"""Voice-conversion models (models/vc): Vevo's autoregressive transformer and flow-matching transformer."""
