/*
 * orx_device.h — gfx950 device-side building blocks of the render core, one header per concern.
 */
#pragma once
#include "orx_rng.h"
#include "orx_isect.h"
#include "orx_traverse.h"
#include "orx_shade.h"
#include "orx_media_dev.h"
