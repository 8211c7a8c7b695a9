// The layout of the three fake-ESPI parameter arrays: espi_params.hip writes them, espi.hip reads them.
#pragma once

#define ESPI_MAX_NODES 7
#define ESPI_NODE_STRIDE 8    // cx, cy, a, b, angle_deg, rings, start (0/1), valid
#define ESPI_WAVE_STRIDE 5    // amp, wavelength, thickness, slope, spacing
