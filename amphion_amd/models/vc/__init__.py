"""Voice-conversion models (models/vc): Vevo's flow-matching transformer."""
