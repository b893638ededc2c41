// TEST INFRASTRUCTURE.  Host half of the ray query API conformance check (see
// rays_conformance.inl): plain host C++, as a simulator's Manager is.
#define RAYSCONF_NAME raysconf_host
#include "rays_conformance.inl"
