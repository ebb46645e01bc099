"""Synthetic data generation, step 2 of the reference's ``synthetic-data-generation/`` on the device: two paired views per label map
(``views``, csrc/amx_synth.hip and csrc/amx_segaug.hip) and its command line
(``python -m anatomix_amd.datagen.step2_generate_views``).  Step 1 (label ensembles) and step 3 (the HDF5 writer) are not here.  MONAI is
not a dependency; its documented algorithms are restated and parity with an installed MONAI is not pinned."""
from .views import (augment_views, clip_rescale, concat_params, draw_fields, draw_params, generate_views, kspace_spike_noise,  # noqa: F401
                    simulate_low_resolution, synthesize_views)
